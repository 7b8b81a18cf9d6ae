"""The elementwise front end (flame_amd/elementwise.py) without a GPU: the three compile limits at
their boundaries, integer scalars that the op's double cannot carry, and the op table of
include/flame_amd.h against the Python constants."""
import os
import re

import pytest
import torch

from flame_amd import elementwise as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "flame_amd.h")


def _nested_sum(k):
    """x*1.0 + (x*2.0 + (... + x*float(k))): every product is computed before the first sum, so k
    products and the new sum, k + 1 values, are live at once."""
    def fn(x):
        terms = [x * float(i + 1) for i in range(k)]
        acc = terms[-1]
        for t in reversed(terms[:-1]):
            acc = t + acc
        return acc
    return fn


def test_live_value_limit_is_exact():
    spec = [(torch.float32, (5,))]
    prog = E.trace(_nested_sum(E.MAX_REGS - 1), spec)            # 32 live values
    assert max(o.dst for o in prog.ops) == E.MAX_REGS - 1
    with pytest.raises(NotImplementedError, match="live values"):
        E.trace(_nested_sum(E.MAX_REGS), spec)                   # 33


def test_op_count_limit_is_exact():
    def chain(n):        # a LOAD, n ADD_S, a STORE
        def fn(x):
            for _ in range(n):
                x = x + 1.0
            return x
        return fn
    spec = [(torch.float32, (5,))]
    assert E.trace(chain(E.MAX_OPS - 2), spec).n_ops == E.MAX_OPS
    with pytest.raises(NotImplementedError, match="ops in one statement"):
        E.trace(chain(E.MAX_OPS - 1), spec)


def test_buffer_limit_is_exact():
    def total(*xs):
        acc = xs[0]
        for x in xs[1:]:
            acc = acc + x
        return acc
    assert E.trace(total, [(torch.int32, (5,))] * (E.MAX_BUFS - 1)).n_in == E.MAX_BUFS - 1    # 15 inputs + 1 output
    with pytest.raises(NotImplementedError, match="buffers in one statement"):
        E.trace(total, [(torch.int32, (5,))] * E.MAX_BUFS)


INT_DTYPES = [torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8, torch.bool]


@pytest.mark.parametrize("dt", INT_DTYPES, ids=[str(d)[6:] for d in INT_DTYPES])
def test_integer_scalar_is_exact_or_refused(dt):
    """An int scalar in an integer dtype (a bool tensor promotes to int64) is carried exactly or the
    statement is refused when it is recorded: 2**53 + 1 is not a double, 2**63 is not an int64."""
    spec = [(dt, (3,))]
    stmts = {"x + s": lambda s: (lambda x: x + s), "s + x": lambda s: (lambda x: s + x),
             "x * s": lambda s: (lambda x: x * s), "s * x": lambda s: (lambda x: s * x)}
    if dt != torch.bool:        # (torch refuses a bool tensor's subtraction)
        stmts["x - s"] = lambda s: (lambda x: x - s)
        stmts["s - x"] = lambda s: (lambda x: s - x)
    for name, mk in stmts.items():
        # (x - 2**63 carries -2**63, an int64, and wraps to what torch-CPU computes)
        for s in (2 ** 53 + 1, -(2 ** 53) - 1, 2 ** 63 - 1, -(2 ** 63) - 1, 2 ** 70, 10 ** 400,
                  -(2 ** 63) if name == "x - s" else 2 ** 63):
            with pytest.raises(NotImplementedError, match="integer scalar"):
                E.trace(mk(s), spec)
        for s in (2 ** 53, -(2 ** 53), 2 ** 62 + 2 ** 38, 300, -3, 0, -(2 ** 63) + 1024):
            prog = E.trace(mk(s), spec)
            # (s - x is recorded as (-x) + s: the MUL_S by -1 aside)
            carried = [int(o.scalar) for o in prog.ops if o.op in (E.ADD_S, E.MUL_S) and o.scalar != -1.0]
            want = -s if name == "x - s" else s
            assert carried == [want], (name, s, carried)
    assert E.trace(lambda x: x + (-(2 ** 63)), spec).n_ops >= 3


def test_bool_subtraction_is_refused_as_torch_refuses_it():
    """torch-CPU refuses every subtraction with a bool tensor (its meta kernels only bool - bool)."""
    b, i = (torch.bool, (3,)), (torch.int8, (3,))
    for fn, spec in ((lambda x, y: x - y, [b, i]), (lambda x, y: x - y, [i, b]), (lambda x, y: x - y, [b, b]),
                     (lambda x: x - 3, [b]), (lambda x: 3 - x, [b]), (lambda x: x - 0.5, [b]), (lambda x: -x, [b])):
        with pytest.raises(RuntimeError) as refused:
            E.trace(fn, spec)
        assert type(refused.value) is RuntimeError
        with pytest.raises(RuntimeError):
            fn(*[torch.ones(sh, dtype=dt) for dt, sh in spec])


def test_integer_scalar_in_a_float_dtype_is_rounded_as_torch_rounds_it():
    """A float dtype takes any int scalar, as torch does (it is rounded to the dtype's opmath)."""
    for dt in (torch.float32, torch.bfloat16, torch.float16, torch.float64):
        prog = E.trace(lambda x: x + (2 ** 53 + 1), [(dt, (3,))])
        assert [o.scalar for o in prog.ops if o.op == E.ADD_S] == [float(2 ** 53 + 1)]


def test_header_op_table_matches_python_constants():
    src = open(HDR).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define FLAME_EW_(\w+)\s+(\d+)", src, flags=re.M)}
    names = ["LOAD", "STORE", "ZERO", "CAST", "ADD", "SUB", "MUL", "DIV", "ADD_S", "MUL_S", "SQUARE", "SIGN", "SQRT"]
    assert [defs.pop(n) for n in names] == list(range(13))
    assert [getattr(E, n) for n in names] == list(range(13))
    assert defs == {"MAX_OPS": E.MAX_OPS, "MAX_REGS": E.MAX_REGS, "MAX_BUFS": E.MAX_BUFS}
    assert sorted(set(E._KIND_OP.values())) == list(range(E.ADD, E.SQRT + 1))
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(
        r"^#define FLAME_(F32|BF16|F16|F64|I64|I32|U8|I8|I16|BOOL)\s+(\d+)", src, flags=re.M)}
    assert sorted(codes.values()) == list(range(10))
    assert {str(dt)[6:]: c for dt, c in E.EW_DTYPES.items()} == {
        "float32": codes["F32"], "bfloat16": codes["BF16"], "float16": codes["F16"], "float64": codes["F64"],
        "int64": codes["I64"], "int32": codes["I32"], "uint8": codes["U8"], "int8": codes["I8"],
        "int16": codes["I16"], "bool": codes["BOOL"]}
    fields = re.search(r"typedef struct flame_ew_op \{(.*?)\} flame_ew_op;", src, flags=re.S).group(1)
    assert re.findall(r"(int32_t|double)\s+(\w+);", fields) == [
        ("int32_t", n) if n != "scalar" else ("double", n) for n, _ in E.EwOp._fields_]
    import ctypes
    assert ctypes.sizeof(E.EwOp) == 32
