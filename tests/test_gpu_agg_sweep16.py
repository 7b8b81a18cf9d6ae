"""GPU: every 16-bit operand through the same-dtype aggregation kernels (flame_agg_reduce,
flame_agg_reduce_scaled, flame_fedbuff_scale_add, flame_hier_fedbuff in FedBuff and sync mode,
flame_feddyn_round), against the torch-CPU restatement of the reference's statements, BITWISE.

Every FedAvg / FedBuff / hierarchy / FedDyn round of a bf16 or fp16 model runs four small functions
of csrc/fedagg.hip -- Tr<>::tmp (the product, rounded to the dtype), Tr<>::add (the sum, rounded to
the dtype), SA<>::op (the quotient, the sum and the delta) and the sync hierarchy's rnd<>(w' - w) --
each instantiated inside another kernel body, which is what decides whether the backend contracts a
product or a quotient with the rounding that follows it (f16_round's empty asm exists because it
once did).  tests/agg_sweep.py holds the operands, the layouts and the expectations:

  * one-operand cases run all 65,536 bit patterns of the dtype (clients beside the first hold
    permutations of them that stay inside each pattern's binade);
  * two-operand cases (the sum, the quotient + sum, the delta, FedDyn's history sum) run the pair
    tensors: 64 accumulators -- every binade with mantissas 0, all-ones and random, both signs, +-0,
    the subnormal range's ends, +-max, +-inf -- x 65,536 patterns = 4,194,304 elements;
  * both layouts: aligned (the vector path; a ragged tail of LANE - 1 elements after the last whole
    chunk runs the per-element bodies) and misaligned (a view one element into its buffer).

Every case goes through flame_amd.engine or the optimizers' public functions, and its launch is
pinned to its kernel by name and by launch branch (agg_sweep.Pinned).  The comparison is
scenarios.same_bits: every non-NaN element bitwise, the sign of zero included; a NaN meets a NaN.
The number of non-NaN expectations per row of patterns is printed and held to agg_sweep.FLOOR
(tests/test_agg_sweep_ref.py establishes that every case keeps it, and holds the restatement itself
to a float64 reference)."""
import itertools

import pytest
import torch

import agg_sweep as A

pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

DT = A.DTYPES16


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


@pytest.mark.parametrize("dt,start,layout", _params(DT, ["acc", "init"], A.LAYOUTS))
def test_reduce_products(dt, start, layout):
    """flame_agg_reduce: RN(v * rate) of three clients (the patterns, two permutations) summed into
    one segment per base; one launch per rate triple, accumulating or from a None start
    (init_first); one launch of 9 clients for the unrolled loop of 8 and its remainder."""
    dtype = DT[dt]
    zeros = [torch.full((A.patterns(dtype).numel(),), b, dtype=dtype) for b in A.bases(dtype)]
    for i, init, n in A.product_launches(dtype):
        if init != (start == "init"):
            continue
        cl, rates, exp = A.cached(("product", dt, i, init, n), lambda: A.product_case(dtype, i, init, n))
        label = f"products/{dt}/{start}/{layout}/launch {i} x {n} clients"
        counts = A.run_reduce(label, dtype, layout, zeros, cl, rates, exp, init_first=init)
        _held(label, dtype, counts)


@pytest.mark.parametrize("dt,layout", _params(DT, A.LAYOUTS))
def test_reduce_sums(dt, layout):
    """flame_agg_reduce: one client at rate 1.0 over the pair tensors, so tmp = v exactly and the
    launch is the dtype's ``acc + v`` on every accumulator x every pattern (bf16: five blocks of 64
    accumulators, one launch each)."""
    dtype = DT[dt]
    for block in range(A.accumulators(dtype).shape[0]):
        acc, pat, exp = A.cached(("sum", dt, block), lambda: A.sum_case(dtype, block))
        label = f"sums/{dt}/{layout}/block {block}"
        _held(label, dtype, A.run_reduce(label, dtype, layout, [acc], [pat], [1.0], [exp]))


@pytest.mark.parametrize("dt,layout", _params(DT, A.LAYOUTS))
def test_reduce_scaled(dt, layout):
    """flame_agg_reduce_scaled: RN(RN(v * scale) * rate) over the scales x three rates on the
    patterns, and one launch over the pair tensors."""
    dtype = DT[dt]
    zeros = [torch.full((A.patterns(dtype).numel(),), b, dtype=dtype) for b in A.bases(dtype)]
    for i in range(len(A.RATES)):
        cl, rates, scales, exp = A.cached(("scaled", dt, i), lambda: A.scaled_case(dtype, i))
        label = f"scaled/{dt}/{layout}/launch {i}"
        _held(label, dtype, A.run_reduce(label, dtype, layout, zeros, cl, rates, exp, scales=scales))
    acc, pat, exp = A.cached(("scaled pair", dt), lambda: A.scaled_pair_case(dtype))
    label = f"scaled/{dt}/{layout}/pair"
    _held(label, dtype, A.run_reduce(label, dtype, layout, [acc], [pat], [A.PAIR_SCALED[1]], [exp],
                                     scales=[A.PAIR_SCALED[0]]))


@pytest.mark.parametrize("dt,goal,layout", _params(DT, A.GOALS, A.LAYOUTS))
def test_scale_add(dt, goal, layout):
    """flame_fedbuff_scale_add: w = the accumulators, a = the patterns; w' = RN(w + RN(a / goal)) and
    delta = RN(w' - w), with and without the delta output.  A delta over an infinite w is NaN
    everywhere (inf - inf): those rows are exempt from the floor, their NaNs still have to be there."""
    dtype = DT[dt]
    w, a, new, delta = A.cached(("scale_add", dt, goal), lambda: A.scale_add_case(dtype, goal))
    fin = A.finite_rows(dtype, A.scale_add_block(dtype, goal))
    for with_delta in (True, False):
        label = f"scale_add/{dt}/goal {goal}/{layout}/{'delta' if with_delta else 'no delta'}"
        cw, cd = A.run_scale_add(label, dtype, layout, w, a, goal, new, delta, with_delta)
        _held(label + "/w", dtype, [cw])
        if with_delta:
            _held(label + "/delta", dtype, [cd], fin)


@pytest.mark.parametrize("dt,mids,start,layout", _params(DT, A.HIER_MIDS, ["none", "accum"], A.LAYOUTS))
def test_hierarchy_fedbuff(dt, mids, start, layout):
    """flame_hier_fedbuff, FedBuff mode: M = 2 (register store groups) and M = 16 (LDS store
    groups), C = 2, goals 3 and 65, constant middle weights from the accumulator list, top_weights
    applied, from a None top aggregate and from an existing one: middle weights, deltas, top
    aggregate and top weights."""
    dtype, M = DT[dt], A.HIER_MIDS[mids]
    o, exp = A.cached(("hier", dt, M, start), lambda: A.hier_expected(dtype, M, False, start == "none"))
    label = f"hierarchy/fedbuff/{dt}/M={M}/{start}/{layout}"
    for nm, counts in A.run_hierarchy(label, dtype, layout, M, start == "none", o, exp).items():
        _held(f"{label}/{nm}", dtype, counts)


@pytest.mark.parametrize("dt,mids,layout", _params(DT, A.HIER_MIDS, A.LAYOUTS))
def test_hierarchy_sync(dt, mids, layout):
    """flame_hier_fedbuff, sync mode: the same shapes under counts that give rates 1/3 and 2/3; the
    delta is rnd(w' - w) on swept w'."""
    dtype, M = DT[dt], A.HIER_MIDS[mids]
    o, exp = A.cached(("hier sync", dt, M), lambda: A.hier_expected(dtype, M, True))
    label = f"hierarchy/sync/{dt}/M={M}/{layout}"
    for nm, counts in A.run_sync_hierarchy(label, dtype, layout, M, o, exp).items():
        _held(f"{label}/{nm}", dtype, counts)


@pytest.mark.parametrize("dt,order,layout", _params(DT, A.DYN_ORDERS, A.LAYOUTS))
def test_feddyn_round(dt, order, layout):
    """flame_feddyn_round: two rounds.  The second one's program has W | AVG | HIN | HOUT | MEAN steps
    whose ``h + w`` is the pair sum (h = the accumulators, w = the patterns) and an HIN | MEAN-only
    end whose history is -0; key "zero" is -0 in every tensor and its cld_model must be +0.  In
    arrival order (the one-phase program) and shuffled (two phases)."""
    dtype = DT[dt]
    operands, rounds = A.cached(("feddyn", dt, order), lambda: A.feddyn_expected(dtype, order))
    label = f"feddyn/{dt}/{order}/{layout}"
    for nm, counts in A.run_feddyn(label, dtype, layout, order, operands, rounds).items():
        _held(f"{label}/{nm}", dtype, counts)
