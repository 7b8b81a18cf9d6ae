"""GPU: the aggregation sweep (tests/test_gpu_agg_sweep16.py) for f32, f64, i32 and i64.

These dtypes have no exhaustive operand list.  f32 and f64 run fedopt_sweep.grid_bits with both
signs -- every exponent field x mantissas 0, 1, the top bit, all-ones and 12 random -- as the
patterns (8,192 and 65,536 values) against a 16-value accumulator list: the reduce products and
sums, the scaled reduction, scale_add with the delta, one hierarchy case per mode (f32: the kernel
carries no f64) and the FedDyn round, whose fourth dtype f64 is.  The same drivers, layouts, pins
and comparison as the 16-bit sweep (tests/agg_sweep.py); the floor is the same share of a row.

i32 / i64 go through flame_agg_reduce only: ``tmp = (v * rate).to(int)`` and the wrapping add, on
+-2^k and +-(2^k +- 1) -- i64 values beyond 2^24 take the int -> fp32 conversion's rounding, negative
products the truncation toward zero -- keeping the operand / rate pairs whose fp32 product fits the
integer type (outside that the reference's cast is undefined behaviour)."""
import itertools

import pytest
import torch

import agg_sweep as A

pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

DT = A.DTYPES_WIDE
INTS = {"i32": torch.int32, "i64": torch.int64}


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    from flame_amd import _native
    _native.lib()
    assert torch.cuda.is_available()
    torch.empty(1, device=A.DEV)


def _params(*lists):
    return [pytest.param(*c, id="-".join(str(x) for x in c)) for c in itertools.product(*lists)]


def _held(label, dtype, counts, keep=None):
    least = A.report(label, dtype, counts, keep)
    assert least >= A.floor(dtype), (label, least)


@pytest.mark.parametrize("dt,layout", _params(DT, A.LAYOUTS))
def test_reduce_products_and_sums(dt, layout):
    dtype = DT[dt]
    segs = [torch.full((A.patterns(dtype).numel(),), b, dtype=dtype) for b in A.bases(dtype)]
    for i, init, n in A.product_launches(dtype):
        cl, rates, exp = A.product_case(dtype, i, init, n)
        label = f"products/{dt}/{'init' if init else 'acc'}/{layout}/launch {i} x {n} clients"
        _held(label, dtype, A.run_reduce(label, dtype, layout, segs, cl, rates, exp, init_first=init))
    acc, pat, exp = A.sum_case(dtype, 0)
    label = f"sums/{dt}/{layout}"
    _held(label, dtype, A.run_reduce(label, dtype, layout, [acc], [pat], [1.0], [exp]))


@pytest.mark.parametrize("dt,layout", _params(DT, A.LAYOUTS))
def test_reduce_scaled(dt, layout):
    dtype = DT[dt]
    segs = [torch.full((A.patterns(dtype).numel(),), b, dtype=dtype) for b in A.bases(dtype)]
    for i in range(4):
        cl, rates, scales, exp = A.scaled_case(dtype, i)
        label = f"scaled/{dt}/{layout}/launch {i}"
        _held(label, dtype, A.run_reduce(label, dtype, layout, segs, cl, rates, exp, scales=scales))
    acc, pat, exp = A.scaled_pair_case(dtype)
    label = f"scaled/{dt}/{layout}/pair"
    _held(label, dtype, A.run_reduce(label, dtype, layout, [acc], [pat], [A.PAIR_SCALED[1]], [exp],
                                     scales=[A.PAIR_SCALED[0]]))


@pytest.mark.parametrize("dt,layout", _params(DT, A.LAYOUTS))
def test_scale_add(dt, layout):
    dtype = DT[dt]
    fin = A.finite_rows(dtype)
    for goal in A.GOALS:
        w, a, new, delta = A.scale_add_case(dtype, goal)
        label = f"scale_add/{dt}/goal {goal}/{layout}"
        cw, cd = A.run_scale_add(label, dtype, layout, w, a, goal, new, delta, True)
        _held(label + "/w", dtype, [cw])
        _held(label + "/delta", dtype, [cd], fin)
    w, a, new, delta = A.scale_add_case(dtype, 3)
    A.run_scale_add(f"scale_add/{dt}/goal 3/{layout}/no delta", dtype, layout, w, a, 3, new, delta, False)


@pytest.mark.parametrize("mode,layout", _params(["fedbuff", "sync"], A.LAYOUTS))
def test_hierarchy_f32(mode, layout):
    dtype, M = torch.float32, A.HIER_MIDS["reg"]
    o, exp = A.hier_expected(dtype, M, mode == "sync", False)
    label = f"hierarchy/{mode}/f32/M={M}/{layout}"
    if mode == "sync":
        res = A.run_sync_hierarchy(label, dtype, layout, M, o, exp)
    else:
        res = A.run_hierarchy(label, dtype, layout, M, False, o, exp)
    for nm, counts in res.items():
        _held(f"{label}/{nm}", dtype, counts)


@pytest.mark.parametrize("dt,order,layout", _params(DT, A.DYN_ORDERS, A.LAYOUTS))
def test_feddyn_round(dt, order, layout):
    dtype = DT[dt]
    operands, rounds = A.cached(("feddyn", dt, order), lambda: A.feddyn_expected(dtype, order))
    label = f"feddyn/{dt}/{order}/{layout}"
    for nm, counts in A.run_feddyn(label, dtype, layout, order, operands, rounds).items():
        _held(f"{label}/{nm}", dtype, counts)


@pytest.mark.parametrize("dt,layout", _params(INTS, A.LAYOUTS))
def test_integer_reduce(dt, layout):
    """One client per launch, one launch per rate, over the kept pairs."""
    dtype = INTS[dt]
    v, base, rates, keep, exp = A.int_case(dtype)
    assert sum(int(k.sum()) for k in keep) >= 0.9 * len(rates) * v.numel()
    for r, k, e in zip(rates, keep, exp):
        label = f"integers/{dt}/{layout}/rate {r}"
        A.run_reduce(label, dtype, layout, [base[k]], [v[k]], [r], [e[k]])
        print(f"{label}: compared {int(k.sum())} of {v.numel()} pairs")
