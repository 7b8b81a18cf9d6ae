"""GPU: the elementwise interpreter (ew_kernel in csrc/fedagg.hip behind flame_amd/elementwise.py)
op by op -- every cast pair, every op on every dtype, scalars, the two launch forms, the grid-stride
loop, the segment lookup, the register allocator -- BITWISE against the same Python function on CPU
tensors.

The reference of an op is its IEEE correctly rounded result:
  * fp32 ``/`` and ``sqrt``: computed in fp64 (numpy) and rounded once to fp32 -- free of
    double-rounding error at 53 bits (torch-CPU's own fp32 sqrt is ~1 ulp off on ~0.6 % of values,
    oracle/oracle.py);
  * bf16 / fp16 ``/`` and ``sqrt``: that fp32 value rounded to the dtype;
  * fp64 arithmetic: numpy float64 ops;
  * everything else: plain torch-CPU.
``_Ref`` wraps a CPU tensor so that one function runs on both sides; it never imports flame_amd.

Excluded inputs -- only where the reference itself is undefined (C++ undefined behaviour), decided
from the INPUT values before anything runs (``_f2i_defined``), never from a result:
  * float -> integer casts of NaN, +inf, -inf (F2I_NONFINITE);
  * float -> integer casts of a finite value whose truncation toward zero is above F2I_LARGEST or
    below F2I_SMALLEST of the target type (torch-CPU returns the x86 "indefinite" value there,
    1e10 -> int32 gives -2147483648; the kernel saturates at int64 and wraps);
  * float -> uint8 casts of a value whose truncation is negative (F2I_SMALLEST[uint8] = 0; no
    product statement depends on it).
Every other input of every case is compared."""
import numpy as np
import pytest
import torch

import scenarios as S
from oracle import consult

pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

DEV = "cuda:0"
F32, BF16, F16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64
I64, I32, I16, I8, U8, BOOL = torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8, torch.bool
DTYPES = [F32, BF16, F16, F64, I64, I32, I16, I8, U8, BOOL]
FLOATS = [F32, BF16, F16, F64]
INTS = [I64, I32, I16, I8, U8]
N_RANDOM = 3000


def _id(dt):
    return str(dt)[6:]


# ------------------------------------------------------------------------------- the reference
class _Ref:
    """A CPU tensor whose ``/`` and ``sqrt`` are correctly rounded and whose fp64 arithmetic is
    numpy's; every other op is torch-CPU's own."""

    def __init__(self, t):
        self.t = t

    dtype = property(lambda self: self.t.dtype)
    shape = property(lambda self: self.t.shape)

    @staticmethod
    def _t(x):
        return x.t if isinstance(x, _Ref) else x

    @staticmethod
    def _np64(fn, *ts):
        with np.errstate(all="ignore"):
            return torch.from_numpy(np.asarray(fn(*[t.contiguous().numpy() for t in ts]), dtype=np.float64).copy())

    def _bin(self, o, fn, npfn, swap=False):
        a, b = (self._t(o), self.t) if swap else (self.t, self._t(o))
        r = fn(a, b)
        if r.dtype == F64 and isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor):
            r = self._np64(npfn, a.to(F64), b.to(F64)).view(r.shape)
        return _Ref(r)

    def __add__(self, o): return self._bin(o, lambda a, b: a + b, np.add)
    def __radd__(self, o): return self._bin(o, lambda a, b: a + b, np.add, swap=True)
    def __sub__(self, o): return self._bin(o, lambda a, b: a - b, np.subtract)
    def __rsub__(self, o): return self._bin(o, lambda a, b: a - b, np.subtract, swap=True)
    def __mul__(self, o): return self._bin(o, lambda a, b: a * b, np.multiply)
    def __rmul__(self, o): return self._bin(o, lambda a, b: a * b, np.multiply, swap=True)
    def __neg__(self): return _Ref(-self.t)
    def __pow__(self, e): return _Ref(self.t ** e)
    def to(self, dt): return _Ref(self.t.to(dt))

    def __truediv__(self, o):
        a, b = self.t, self._t(o)
        dt = (a[..., :0] / b[..., :0]).dtype if a.dim() else (a.new_zeros(()) / b.new_zeros(())).dtype
        q = self._np64(np.divide, a.to(dt).to(F64), b.to(dt).to(F64)).view(a.shape)      # operands in the op's dtype first
        return _Ref(q if dt == F64 else q.to(F32).to(dt))

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        x = args[0].t
        if func is torch.sqrt:
            dt = torch.sqrt(x[..., :0] if x.dim() else x.new_zeros(())).dtype
            r = cls._np64(np.sqrt, x.to(dt).to(F64)).view(x.shape)
            return _Ref(r if dt == F64 else r.to(F32).to(dt))
        if func in (torch.sign, torch.zeros_like):
            return _Ref(func(x))
        raise NotImplementedError(func)


def _reference(fn, xs):
    """``fn`` on CPU tensors (``_Ref``): a checker (oracle/consult.py)."""
    consult.note()
    out = fn(*[_Ref(x) for x in xs])
    outs = list(out) if isinstance(out, (tuple, list)) else [out]
    return [o.t for o in outs]


def _kernel(fn, xs):
    from flame_amd import elementwise as E
    prog = E.trace(fn, [(x.dtype, tuple(x.shape)) for x in xs])
    return prog(*[x.to(DEV) for x in xs], device=torch.device(DEV))


def _check(label, fn, xs):
    """fn on the kernel against fn on the reference, every output, bitwise."""
    exp = _reference(fn, xs)
    got = _kernel(fn, xs)
    assert len(got) == len(exp), label
    S.same_bits(label, {i: g for i, g in enumerate(got)}, {i: e for i, e in enumerate(exp)})


def _check_each(label, stmts, xs):
    """Named one-output statements: one that the reference refuses (RuntimeError) must be refused
    when it is recorded; the others run as ONE program with two outputs each: the result, and the
    result widened to fp64 (what a later op reads from the register, which must already be wrapped
    or rounded to the dtype, not only what the store narrows)."""
    from flame_amd import elementwise as E
    ok = []
    for name, fn in stmts:
        try:
            _reference(fn, xs)
        except RuntimeError:
            with pytest.raises(RuntimeError) as refused:
                E.trace(fn, [(x.dtype, tuple(x.shape)) for x in xs])
            assert type(refused.value) is RuntimeError, refused.value       # torch's own error, not a missing feature
            continue
        ok.append((name, fn))
    for i in range(0, len(ok), 6):      # a few outputs per program (MAX_BUFS)
        part = ok[i:i + 6]
        names = [n + w for n, _ in part for w in ("", " -> fp64")]

        def both(*a):
            return [o for _, fn in part for r in [fn(*a)] for o in (r, r.to(F64))]
        exp, got = _reference(both, xs), _kernel(both, xs)
        S.same_bits(label, dict(zip(names, got)), dict(zip(names, exp)))


# ------------------------------------------------------------------------------------ inputs
INF, NAN = float("inf"), float("nan")
# float edge values (given as doubles; a narrower dtype takes them rounded)
FLOAT_EDGES = [
    0.0, -0.0, 0.5, -0.5, 0.9, -0.9, 1.0, -1.0, 1.5, 2.5, -2.5, 3.0, 3.999, 100.75, -100.75, 127.0, -128.0, 200.5,
    254.5, 255.0, 300.0, -300.0, 32512.0, -32768.0, 65504.0, 65519.0, 65520.0, -65520.0, 65536.0, 1e5,
    16777217.0, 2.0 ** 31 - 128, -2.0 ** 31, 1e10, 2.0 ** 62, -2.0 ** 63, 2.0 ** 63, 1e19,
    # fp64 -> fp16 through fp32 differs from the direct rounding (the first must give 1.0)
    1 + 2.0 ** -11 + 2.0 ** -30, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11 - 2.0 ** -30, -(1 + 2.0 ** -11 + 2.0 ** -30),
    1 + 2.0 ** -11 - 2.0 ** -30, 2.0 ** -24 * (0.5 + 2.0 ** -30),
    # ... and fp64 -> bf16
    1 + 2.0 ** -8 + 2.0 ** -30, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8 - 2.0 ** -30, -(1 + 2.0 ** -8 + 2.0 ** -30),
    1 + 2.0 ** -8 - 2.0 ** -30, 3.0 * 2.0 ** 100 * (1 + 2.0 ** -8 + 2.0 ** -30),
    # fp32 subnormals, the fp32 / bf16 subnormal boundary and rounding ties below it
    1e-40, -1e-40, 2.0 ** -149, 2.0 ** -150, 2.0 ** -150 * (1 + 2.0 ** -20), 2.0 ** -126, 2.0 ** -127, 1e-39,
    2.0 ** -133, 2.0 ** -134, 2.0 ** -134 * (1 + 2.0 ** -20), 3 * 2.0 ** -134,
    # fp16 subnormals and the boundary
    2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -10), 3 * 2.0 ** -25, 6e-8, -6e-8, 6.1e-5, 2.0 ** -14, 2.0 ** -15,
    2.0 ** -14 * (1 - 2.0 ** -12),
    # fp64 subnormals and extremes; the fp32 / bf16 overflow boundaries (largest value, the tie, just under it)
    5e-324, 1e-310, -1e-310, 1e-300, 1e300, -1e308, 1.7976931348623157e308,
    3.4028234663852886e38, 3.4028235677973366e38, 3.4028235677973362e38, -3.4028235677973366e38,
    3.3895313892515355e38, 3.3961775292304601e38, 3.396177529230460e38 * (1 - 2.0 ** -40), 3.4e38,
    INF, -INF, NAN]
# (what of FLOAT_EDGES a float -> integer cast leaves out; see the module docstring)
F2I_NONFINITE = [INF, -INF, NAN]
F2I_LARGEST = {I8: 127, U8: 255, I16: 32767, I32: 2 ** 31 - 1, I64: 2 ** 63 - 1}     # a truncation above: undefined
F2I_SMALLEST = {I8: -128, U8: 0, I16: -32768, I32: -(2 ** 31), I64: -(2 ** 63)}       # ... or below (uint8: negative)
INT_EDGES = [0, 1, -1, 2, 3, 5, -7, 127, 128, -128, -129, 200, 255, 256, 300, 32767, 32768, -32768, -32769, 65504,
             65519, 65520, 65535, 65536, 2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24) - 1, 2 ** 31 - 1, 2 ** 31, -(2 ** 31),
             -(2 ** 31) - 1, 2 ** 32 + 5, 2 ** 53 + 1, 2 ** 62 + 2 ** 38 + 1, 2 ** 62 + 2 ** 38, 2 ** 62 + 2 ** 39 + 1,
             2 ** 63 - 1, -(2 ** 63), -(2 ** 63) + 1, 2 ** 63 - 2 ** 39, 2 ** 63 - 2 ** 39 - 1]


def _int_range(dt):
    return (0, 255) if dt == U8 else (torch.iinfo(dt).min, torch.iinfo(dt).max)


def _rand_floats(rng, dt, n):
    """sign * [1, 2) * 2^e: half with e over the dtype's whole range (subnormals, overflow), half near 1."""
    lo, hi = {F16: (-26, 16), BF16: (-136, 128), F32: (-151, 128), F64: (-1076, 1024)}[dt]
    e = np.where(rng.random(n) < 0.5, rng.integers(lo, hi, n), rng.integers(-12, 12, n))
    with np.errstate(over="ignore"):
        v = np.ldexp(1.0 + rng.random(n), e) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    return torch.from_numpy(v).to(dt)


def _rand_ints(rng, dt, n):
    lo, hi = _int_range(dt)
    wide = torch.from_numpy(rng.integers(lo, hi, n, dtype=np.int64, endpoint=True))
    near = torch.from_numpy(rng.integers(max(lo, -300), min(hi, 300), n, dtype=np.int64, endpoint=True))
    return torch.where(torch.from_numpy(rng.random(n) < 0.5), wide, near).to(dt)


def _edges(dt):
    if dt == BOOL:
        return torch.tensor([True, False, False, True])
    if dt.is_floating_point:
        return torch.tensor(FLOAT_EDGES, dtype=F64).to(dt)
    lo, hi = _int_range(dt)
    return torch.tensor([v for v in INT_EDGES if lo <= v <= hi], dtype=I64).to(dt)


def _values(dt, seed, n=N_RANDOM):
    rng = np.random.default_rng(seed)
    if dt == BOOL:
        return torch.cat([_edges(dt), torch.from_numpy(rng.random(n) < 0.4)])
    return torch.cat([_edges(dt), (_rand_floats if dt.is_floating_point else _rand_ints)(rng, dt, n)])


def _f2i_defined(x, dst):
    """Which elements of the float tensor x a cast to the integer dtype dst is defined for."""
    t = torch.trunc(x.to(F64))          # (both bounds are exact doubles: a power of two, or below 2^53)
    return torch.isfinite(t) & (t >= float(F2I_SMALLEST[dst])) & (t < float(F2I_LARGEST[dst] + 1))


def _cast_inputs(src, dst, seed):
    x = _values(src, seed)
    if src.is_floating_point and not dst.is_floating_point and dst != BOOL:
        top = float(torch.finfo(src).max)
        lo, hi = max(F2I_SMALLEST[dst], -top), min(F2I_LARGEST[dst], top)
        rng = np.random.default_rng(seed + 1)
        # (random values inside the target's and the source's range: 0.99 keeps a 16-bit rounding inside too)
        inside = torch.from_numpy(rng.uniform(lo * 0.99, hi * 0.99, N_RANDOM)).to(src)
        x = torch.cat([x, inside])
        x = x[_f2i_defined(x, dst)]
    return x


# ------------------------------------------------------------------------------------- casts
PAIRS = [(s, d) for s in DTYPES for d in DTYPES if s != d]
assert len(PAIRS) == 90


@pytest.mark.parametrize("src,dst", PAIRS, ids=[f"{_id(s)}-{_id(d)}" for s, d in PAIRS])
def test_cast_matrix(src, dst):
    x = _cast_inputs(src, dst, 100 + DTYPES.index(src) * 10 + DTYPES.index(dst))
    assert x.numel() > N_RANDOM // 2
    # (and the cast's value as a later op reads it: widened to fp64, or to int64 from fp64)
    wide = I64 if F64 in (src, dst) and not dst.is_floating_point else F64
    _check(f"{_id(src)}->{_id(dst)}", lambda a: (a.to(dst), a.to(dst).to(wide)), [x])


def test_cast_matrix_named_values():
    """The values the cast matrix must hold, spelled out (the reference's results are asserted
    too, so a change of torch's would show here and not as a kernel failure)."""
    def both(x, dst, want):
        exp = _reference(lambda a: a.to(dst), [x])[0]
        assert exp.tolist() == want, (exp.tolist(), want)
        _check(f"{x.dtype}->{dst}", lambda a: a.to(dst), [x])
    both(torch.tensor([1 + 2.0 ** -11 + 2.0 ** -30, 65520.0, 65519.0], dtype=F64), F16, [1.0, INF, 65504.0])
    both(torch.tensor([1 + 2.0 ** -8 + 2.0 ** -30], dtype=F64), BF16, [1.0])
    both(torch.tensor([-(2 ** 31) - 1, 2 ** 32 + 5, -129], dtype=I64), I32, [2147483647, 5, -129])
    both(torch.tensor([-129, 200, 2 ** 62 + 2 ** 38 + 1], dtype=I64), I8, [127, -56, 1])
    both(torch.tensor([-129, 300, -1], dtype=I64), U8, [127, 44, 255])
    both(torch.tensor([2 ** 24 + 1, 2 ** 62 + 2 ** 38 + 1, 2 ** 63 - 1, -(2 ** 63)], dtype=I64), F32,
         [16777216.0, 2.0 ** 62 + 2.0 ** 39, 2.0 ** 63, -2.0 ** 63])
    both(torch.tensor([2 ** 24 + 1, 65520, 65519], dtype=I64), F16, [INF, INF, 65504.0])
    both(torch.tensor([-0.0, 0.5, -0.9, NAN, 0.0], dtype=F32), BOOL, [False, True, True, True, False])
    for dt in INTS:
        both(torch.tensor([-0.0, -0.9, 0.9, 3.999], dtype=F64), dt, [0, 0, 0, 3])
    both(torch.tensor([2.0 ** -24, 2.0 ** -25 * (1 + 2.0 ** -10), 6e-8], dtype=F16), F32,
         [2.0 ** -24, 2.0 ** -24, 2.0 ** -24])


# ---------------------------------------------------------------------------- binary ops
def _float_pair_edges(dt):
    fi = torch.finfo(dt)
    ulp_max = fi.max * fi.eps / (2 - fi.eps) if dt != F64 else 2.0 ** 971       # the top binade's spacing
    tiny_sub = {F16: 2.0 ** -24, BF16: 2.0 ** -133, F32: 2.0 ** -149, F64: 5e-324}[dt]
    v = [0.0, -0.0, 1.0, -1.0, 3.0, 0.1, -7.5, 1.5, 1 + fi.eps, 1 + 2 * fi.eps, 1 - fi.eps / 2, fi.eps / 2, fi.eps / 4,
         3 * fi.eps / 4, -fi.eps / 2, fi.tiny, -fi.tiny, 1.5 * fi.tiny, fi.tiny * (1 + fi.eps), tiny_sub, -tiny_sub,
         3 * tiny_sub, fi.tiny / 2, fi.max, -fi.max, fi.max / 2, fi.max / 2 * (1 + fi.eps), ulp_max / 2, ulp_max / 4,
         -ulp_max / 2, 3 * ulp_max / 4, 2.0 ** (fi.bits // 2), 1 / 3, INF, -INF, NAN]
    t = torch.tensor(v, dtype=F64).to(dt)
    return t.repeat_interleave(len(v)), t.repeat(len(v))


def _int_pair_edges(dt):
    lo, hi = _int_range(dt)
    v = sorted({lo, lo + 1, hi, hi - 1, 0, 1, 2, 3, 5, 100, min(hi, 200)} | ({-1, -3, -128} if lo < 0 else set()))
    t = torch.tensor(v, dtype=I64).to(dt)
    return t.repeat_interleave(len(v)), t.repeat(len(v))


def _pair(dt, seed):
    rng = np.random.default_rng(seed)
    if dt == BOOL:
        a, b = torch.tensor([True, True, False, False]), torch.tensor([True, False, True, False])
        return torch.cat([a, torch.from_numpy(rng.random(500) < 0.5)]), torch.cat([b, torch.from_numpy(rng.random(500) < 0.5)])
    ea, eb = (_float_pair_edges if dt.is_floating_point else _int_pair_edges)(dt)
    r = _rand_floats if dt.is_floating_point else _rand_ints
    return torch.cat([ea, r(rng, dt, N_RANDOM)]), torch.cat([eb, r(rng, dt, N_RANDOM)])


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_binary_same_dtype(dt):
    a, b = _pair(dt, 300 + DTYPES.index(dt))
    stmts = [("a + b", lambda x, y: x + y), ("a - b", lambda x, y: x - y), ("a * b", lambda x, y: x * y)]
    if dt != BOOL:
        stmts.append(("a / b", lambda x, y: x / y))         # int / int promotes to fp32
        # an op on a wrapped / rounded result
        stmts += [("sign(a * b)", lambda x, y: torch.sign(x * y)), ("(a - b) / b", lambda x, y: (x - y) / y),
                  ("(a + b) * b", lambda x, y: (x + y) * y)]
    if dt == BOOL:
        from flame_amd import elementwise as E
        with pytest.raises(RuntimeError):                   # as torch: refused when recorded
            E.trace(lambda x, y: x - y, [(BOOL, (4,)), (BOOL, (4,))])
    _check_each(f"{_id(dt)} binary", stmts, [a, b])


def test_binary_named_values():
    def both(fn, xs, want):
        exp = _reference(fn, xs)[0]
        assert exp.tolist() == want, (exp.tolist(), want)
        _check("named", fn, xs)
    both(lambda a, b: a * b, [torch.tensor([-(2 ** 31)], dtype=I32), torch.tensor([-1], dtype=I32)], [-(2 ** 31)])
    both(lambda a, b: a * b, [torch.tensor([-(2 ** 63)], dtype=I64), torch.tensor([-1], dtype=I64)], [-(2 ** 63)])
    both(lambda a, b: a - b, [torch.tensor([-128], dtype=I8), torch.tensor([1], dtype=I8)], [127])
    both(lambda a, b: a * b, [torch.tensor([200], dtype=U8), torch.tensor([200], dtype=U8)], [64])
    both(lambda a, b: a - b, [torch.tensor([3], dtype=U8), torch.tensor([5], dtype=U8)], [254])
    both(lambda a, b: a + b, [torch.tensor([65504.0, 65504.0], dtype=F16), torch.tensor([16.0, 8.0], dtype=F16)],
         [INF, 65504.0])
    both(lambda a, b: a + b, [torch.tensor([1.0, 1.0], dtype=BF16), torch.tensor([2.0 ** -8, 3 * 2.0 ** -8], dtype=BF16)],
         [1.0, 1.015625])


MIXED = [(I64, F32), (BF16, F16), (U8, I8), (I32, F64), (BOOL, I8), (F16, I64), (F64, F32), (I16, U8), (I8, BF16),
         (F32, I64)]


@pytest.mark.parametrize("da,db", MIXED, ids=[f"{_id(a)}-{_id(b)}" for a, b in MIXED])
def test_binary_mixed_dtype(da, db):
    a, b = _values(da, 400 + DTYPES.index(da)), _values(db, 420 + DTYPES.index(db))
    n = min(a.numel(), b.numel())
    ea, eb = _edges(da), _edges(db)
    a = torch.cat([ea.repeat_interleave(len(eb)), a[-n:]])      # every edge against every edge, then random
    b = torch.cat([eb.repeat(len(ea)), b[-n:]])
    stmts = [("a + b", lambda x, y: x + y), ("a - b", lambda x, y: x - y), ("b - a", lambda x, y: y - x),
             ("a * b", lambda x, y: x * y), ("a / b", lambda x, y: x / y)]
    _check_each(f"{_id(da)} x {_id(db)}", stmts, [a, b])


@pytest.mark.parametrize("dt", [I64, F32], ids=_id)
def test_binary_zero_dim(dt):
    stmts = [("a + b", lambda x, y: x + y), ("a - b", lambda x, y: x - y), ("a * b", lambda x, y: x * y),
             ("a / b", lambda x, y: x / y)]
    for va, vb in [(7, -3), (2 ** 24 + 1, 3), (0, 0)]:
        _check_each(f"0-dim {_id(dt)}", stmts, [torch.tensor(va, dtype=dt), torch.tensor(vb, dtype=dt)])
    # a 0-dim int64 with a 0-dim fp32: both 0-dim, so the float wins
    _check_each("0-dim int64 x fp32", stmts, [torch.tensor(2 ** 24 + 1, dtype=I64), torch.tensor(0.3, dtype=F32)])


# ---------------------------------------------------------------------------- scalar ops
SCALARS = [1e-3, 0.1, 1.001, -3, 300, 2 ** 31, 0]


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_scalar_ops(dt):
    x = _values(dt, 500 + DTYPES.index(dt))
    for s in SCALARS:
        stmts = [("x + s", lambda a: a + s), ("s + x", lambda a: s + a), ("x - s", lambda a: a - s),
                 ("s - x", lambda a: s - a), ("x * s", lambda a: a * s), ("s * x", lambda a: s * a)]
        _check_each(f"{_id(dt)} scalar {s}", stmts, [x])
    _check_each(f"{_id(dt)} neg", [("-x", lambda a: -a)], [x])


def test_scalar_named_values():
    """1.001 on bf16 separates "round the scalar first" (+) from "fp32 opmath" (*)."""
    x = torch.tensor([1, 256, 0.3], dtype=BF16)
    assert _reference(lambda a: a + 1.001, [x])[0].tolist() == [2.0, 256.0, 1.296875]
    assert _reference(lambda a: a * 1.001, [x])[0].tolist() == [1.0, 256.0, 0.30078125]
    _check("bf16 +- 1.001", lambda a: (a + 1.001, a * 1.001, 1.001 - a, a - 1.001), [x])
    u = torch.tensor([1, 0, 3, 250], dtype=U8)
    assert _reference(lambda a: a + 300, [u])[0].tolist() == [45, 44, 47, 38]
    _check("uint8 + 300", lambda a: (a + 300, a * 300, 300 - a, -a), [u])


# ----------------------------------------------------------------------------- unary ops
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_unary_ops(dt):
    x = _values(dt, 600 + DTYPES.index(dt))
    stmts = [("x ** 2", lambda a: a ** 2), ("sign", lambda a: torch.sign(a)), ("sqrt", lambda a: torch.sqrt(a)),
             ("zeros_like", lambda a: torch.zeros_like(a))]
    _check_each(f"{_id(dt)} unary", stmts, [x])
    if dt.is_floating_point:
        z = torch.tensor([NAN, 0.0, -0.0, -INF, -2.0, INF, 4.0], dtype=dt)
        sg, rt = _reference(lambda a: (torch.sign(a), torch.sqrt(a)), [z])
        assert sg.tolist() == [0.0, 0.0, 0.0, -1.0, -1.0, 1.0, 1.0] and not torch.signbit(sg[:3]).any()
        assert torch.isnan(rt[[0, 3, 4]]).all() and rt[1:3].tolist() == [0.0, -0.0] and bool(torch.signbit(rt[2]))
        _check(f"{_id(dt)} sign / sqrt edges", lambda a: (torch.sign(a), torch.sqrt(a)), [z])


# ------------------------------------------------------------------- division / root sweeps
def _sweep_operands(dt, seed, n):
    """n (a, b) pairs: random significands; exponents over the whole range, then clusters within
    +-2 binades of each switch point for an operand and for the quotient."""
    rng = np.random.default_rng(seed)
    if dt == F64:
        emin, emax, points = -1074, 1023, [-960, 960, -900, -1022, 1023]
    else:
        emin, emax, points = -149, 127, [-126, 127]
    # (quotient clusters: a's exponent minus b's within +-2 of the point and of the subnormal range's end)
    qpoints = points + [emin, emax + 1]
    kinds = rng.integers(0, 4, n)
    jit = rng.integers(-2, 3, n)
    ea = rng.integers(emin - 1, emax + 1, n)
    eb = rng.integers(emin - 1, emax + 1, n)
    p = np.asarray(points)[rng.integers(0, len(points), n)]
    q = np.asarray(qpoints)[rng.integers(0, len(qpoints), n)]
    mod = rng.integers(-40, 40, n)
    ea = np.where(kinds == 1, p + jit, ea)                      # a at a switch point, b modest
    eb = np.where(kinds == 1, mod, eb)
    ea = np.where(kinds == 2, q // 2 + mod, ea)                 # the quotient at one: ea - eb = q + jit
    eb = np.where(kinds == 2, q // 2 + mod - q - jit, eb)
    ea = np.where(kinds == 3, mod, ea)                          # b at a switch point, a modest
    eb = np.where(kinds == 3, p + jit, eb)
    def make(e):
        with np.errstate(all="ignore"):
            return np.ldexp(1.0 + rng.random(n), e) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    return torch.from_numpy(make(ea)).to(dt), torch.from_numpy(make(eb)).to(dt)


def _sweep(dt, seed):
    n, chunk = 1 << 18, 1 << 16
    from flame_amd import elementwise as E
    fn = lambda a, b, x: (a / b, torch.sqrt(x))     # noqa: E731
    prog = E.trace(fn, [(dt, (chunk,))] * 3)
    seen = {"sub_q": 0, "inf_q": 0, "sub_in": 0}
    tiny = torch.finfo(dt).tiny
    for c in range(n // chunk):
        a, b = _sweep_operands(dt, seed + c, chunk)
        x = a.abs()
        exp = _reference(fn, [a, b, x])
        got = prog(a.to(DEV), b.to(DEV), x.to(DEV), device=torch.device(DEV))
        S.same_bits(f"{_id(dt)} sweep chunk {c}", {"a / b": got[0], "sqrt": got[1]}, {"a / b": exp[0], "sqrt": exp[1]})
        seen["sub_q"] += int(((exp[0].abs() < tiny) & (exp[0] != 0)).sum())
        seen["inf_q"] += int(torch.isinf(exp[0]).sum())
        seen["sub_in"] += int(((x < tiny) & (x != 0)).sum())
    assert min(seen.values()) > 1000, seen       # the sweep did hold subnormal and overflowing quotients


def test_fp64_div_sqrt_sweep():
    _sweep(F64, 7000)


def test_fp32_div_sqrt_sweep():
    _sweep(F32, 7100)


# ------------------------------------------------------------------------------ launch forms
CAP = 4096 * 256        # the grid cap of both entry points, in lanes
SENTINEL = -0x0123456789ABCDEF


def _index_fn(x, y):
    return x * 3 + 7 + y


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, CAP - 1, CAP, CAP + 1, 2 * CAP + 77])
def test_long_launch_grid_stride(n):
    """A result that depends on the element's own index, written into a view of a sentinel-filled
    buffer: every element written, nothing outside it."""
    from flame_amd import elementwise as E
    dev = torch.device(DEV)
    x = torch.arange(n, dtype=I64)
    y = (torch.arange(n, dtype=I64) * 2654435761) % 1000003
    exp = _reference(_index_fn, [x, y])[0]
    prog = E.trace(_index_fn, [(I64, (n,))] * 2)
    xd, yd = x.to(dev), y.to(dev)
    S.same_bits(f"flame_elementwise n={n}", {"out": prog(xd, yd, device=dev)[0]}, {"out": exp})
    pad = 300
    buf = torch.full((n + 2 * pad,), SENTINEL, dtype=I64, device=dev)
    out = buf[pad:pad + n]
    prog.run_many([(xd, yd)], dev, into=[[out]])
    S.same_bits(f"flame_elementwise_segments n={n}", {"out": out}, {"out": exp})
    assert bool((buf[:pad] == SENTINEL).all()) and bool((buf[pad + n:] == SENTINEL).all())


def _seg_fn(x, y):
    return x * 3 + y, (x - y).to(I32), x.to(F32) / y.to(F32)


def _rows(shapes):
    """Per row (x, y): the row's number in every element."""
    rows = []
    for r, sh in enumerate(shapes):
        n = int(np.prod(sh, dtype=np.int64))
        x = (torch.arange(n, dtype=I64) + (r + 1) * 1000003).view(sh)
        y = (torch.arange(n, dtype=I64) % 7 + (r + 1)).view(sh)
        rows.append((x, y))
    return rows


def _seg_check(label, got, rows):
    assert len(got) == len(rows)
    for r, (row, g) in enumerate(zip(rows, got)):
        exp = _reference(_seg_fn, list(row))
        assert len(g) == len(exp)
        S.same_bits(f"{label} row {r}", dict(enumerate(g)), dict(enumerate(exp)))


LENGTHS = [0, 1, 255, 0, 257, 1, 70000, 0]


def test_segments():
    from flame_amd import _native
    from flame_amd import elementwise as E
    dev = torch.device(DEV)
    prog = E.trace(_seg_fn, [(I64, (5,))] * 2)
    prog0 = E.trace(_seg_fn, [(I64, ())] * 2)           # (a program is traced per 0-dim-ness)
    out_dt = [I64, I32, F32]

    def dev_rows(rows):
        return [tuple(t.to(dev) for t in row) for row in rows]

    def launches():
        return _native.launch_branch_counts()["flame_elementwise_segments"]

    # the table path: zero-length rows first, in the middle and last; boundaries inside a wavefront
    rows = _rows([(n,) for n in LENGTHS])
    before = launches()
    _seg_check("lengths", prog.run_many(dev_rows(rows), dev), rows)
    assert launches() == before + 1
    # the same into adjacent views of one sentinel-padded buffer per output
    pad, total = 64, sum(LENGTHS)
    bufs = [torch.full((total + 2 * pad,), 77, dtype=dt, device=dev) for dt in out_dt]
    into, off = [], pad
    for n in LENGTHS:
        into.append([b[off:off + n] for b in bufs])
        off += n
    got = prog.run_many(dev_rows(rows), dev, into=into)
    assert all(g.data_ptr() == t.data_ptr() for grow, trow in zip(got, into) for g, t in zip(grow, trow))
    _seg_check("lengths into", into, rows)
    for b in bufs:
        assert bool((b[:pad] == 77).all()) and bool((b[pad + total:] == 77).all())
    # 300 rows of one element; 0-dim rows; 2-d rows
    for label, shapes in (("300 x 1", [(1,)] * 300), ("0-dim", [()] * 5), ("2-d", [(3, 5), (1, 1), (0, 4), (2, 129)])):
        rows = _rows(shapes)
        got = (prog0 if label == "0-dim" else prog).run_many(dev_rows(rows), dev)
        assert [tuple(g[0].shape) for g in got] == [tuple(s) for s in shapes]
        _seg_check(label, got, rows)
    # in place: the first output written over the row's x (element i is read before it is written)
    rows = _rows([(n,) for n in (257, 0, 1, 4099)])
    drows = dev_rows(rows)
    into = [[x, torch.empty(x.shape, dtype=I32, device=dev), torch.empty(x.shape, dtype=F32, device=dev)] for x, _ in drows]
    prog.run_many(drows, dev, into=into)
    _seg_check("in place", into, rows)
    # an all-empty call: no launch, empty outputs
    rows = _rows([(0,), (0, 3), (0,)])
    before = launches()
    got = prog.run_many(dev_rows(rows), dev)
    assert launches() == before and [[o.numel() for o in g] for g in got] == [[0, 0, 0]] * 3
    assert [tuple(g[0].shape) for g in got] == [(0,), (0, 3), (0,)]
    assert [o.dtype for o in got[0]] == out_dt
    assert prog.run_many([], dev) == []
    # the one-row shortcut (flame_elementwise) and one row through the table (into)
    rows = _rows([(1031,)])
    before = launches()
    _seg_check("one row", prog.run_many(dev_rows(rows), dev), rows)
    assert launches() == before
    into = [[torch.empty(1031, dtype=dt, device=dev) for dt in out_dt]]
    prog.run_many(dev_rows(rows), dev, into=into)
    assert launches() == before + 1
    _seg_check("one row into", into, rows)


# --------------------------------------------------------------------- the register allocator
def test_register_pressure():
    from flame_amd import elementwise as E

    def fn(x):          # x*1.0 + (x*2.0 + (... + x*26.0)): every product is live before the first sum
        terms = [x * float(i + 1) for i in range(26)]
        acc = terms[-1]
        for t in reversed(terms[:-1]):
            acc = t + acc
        return acc
    x = _values(F32, 800)
    prog = E.trace(fn, [(F32, tuple(x.shape))])
    assert max(op.dst for op in prog.ops) >= 23
    exp = _reference(fn, [x])
    got = prog(x.to(DEV), device=torch.device(DEV))
    S.same_bits("26 live products", dict(enumerate(got)), dict(enumerate(exp)))


# -------------------------------------------------------------------------------- in-place add
IADD = [(F16, F32), (BF16, F64), (U8, I64), (I64, I32), (F32, I64)]


def _iadd_reference(target, addend):
    """torch-CPU's own ``target += addend``: a checker."""
    consult.note()
    target += addend
    return target


@pytest.mark.parametrize("dt,da", IADD, ids=[f"{_id(t)}-{_id(a)}" for t, a in IADD])
def test_iadd_in_place(dt, da):
    from flame_amd import elementwise as E
    t0, a0 = _values(dt, 900 + DTYPES.index(dt)), _values(da, 920 + DTYPES.index(da))
    n = min(t0.numel(), a0.numel())
    et, ea = _edges(dt), _edges(da)
    t0 = torch.cat([et.repeat_interleave(len(ea)), t0[-n:]])
    a0 = torch.cat([ea.repeat(len(et)), a0[-n:]])
    exp = _iadd_reference(t0.clone(), a0)
    # a contiguous device target: written directly
    t = t0.to(DEV)
    ptr = t.data_ptr()
    E.iadd(t, E.Lazy.of(a0.to(DEV)))
    assert t.data_ptr() == ptr
    S.same_bits(f"{_id(dt)} += {_id(da)}", {"t": t}, {"t": exp})
    # a non-contiguous one: every other element of a buffer, the rest untouched
    base = torch.zeros(2 * t0.numel(), dtype=dt, device=DEV)
    base[1::2] = 1
    view = base[::2]
    view.copy_(t0)
    assert not view.is_contiguous()
    E.iadd(view, E.Lazy.of(a0.to(DEV)))
    S.same_bits(f"{_id(dt)} += {_id(da)} strided", {"t": base[::2]}, {"t": exp})
    assert bool((base[1::2] == 1).all())
