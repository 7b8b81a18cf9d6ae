"""GPU: every 16-bit operand through the shipped FedOPT step kernels (adapt_vec_half, adapt_elem,
fedopt_chain_body, fedopt_chain_body_f16 and csrc/fastmath.h), against OracleFedOPT, BITWISE.

The fast paths of the 16-bit steps stand on claims of the form "equal on every operand": the
hardware root under the bf16 / fp16 rounding, num * v_rcp_f32 under the bf16 rounding, the packed
fp16 root, signed zeros through the mixed-precision products, FedYogi's sign on every sign, zero and
NaN.  A 16-bit dtype has 65,536 values and the optimizer's state is assignable, so the library's
own entry points run them all (tests/fedopt_sweep.py: the operand injection, the lane packings and
the layouts):

  * root sweep: v = every bit pattern, one ordinary m, at tau = the admission bounds, values
    inside and one value just outside each bound;
  * quotient sweep: m = every bit pattern x the v list of fedopt_sweep.quotient_v_bits (+0, the
    smallest and the largest subnormal, every binade up to the largest admitted v with mantissas 0,
    all-ones and random; the slots beyond that hold squares of short roots, whose dens make exact
    midpoint quotients possible).  fp16: 128 values, one launch of 8.4 M elements (two where lanes
    are poisoned).  bf16 has 205 binades of normals up to 2^78, more than 128 values can cover one
    by one, so its list has 224 values and a case takes two launches of at most 16 MB per tensor;
  * moment sweep: the client's update d = every bit pattern x 64 (m, v) states, under the default
    hyperparameters and beta_1 = 0.5, beta_2 = 1.25, eta = 4, tau = 1024.

Each through both kernels (the per-call fused launch and the deferred eager chain, pinned by the
launch-branch counters), both layouts (whole aligned chunks: the vector path, for the fp16 chain the
packed body; a view one element into its buffer: the per-element path) and the lane packings (every
lane admitted; every lane holding one v = +inf, so that the sweep runs the general sequences; every
other lane, so that both sides run exec-masked in each wave).

The comparison is test_gpu_fastmath.py's: NaN positions equal, every other element bitwise equal
(the sign of zero included), on current, m_t and v_t; the elements compared bitwise are counted so
that the NaN exclusion cannot hide a failure.  The expectation itself is checked against a plain
float64 reference in tests/test_fedopt_sweep_ref.py.  The oracle's step is elementwise, so it runs
once per (dtype, variant, hyperparameters) on the sweep's source and is shared by the packings,
layouts and kernels of that sweep."""
import functools
import itertools

import pytest
import torch

import fedopt_sweep as F

pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

DEV = "cuda:0"
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
UPPER = {"bf16": 2.0 ** 38, "f16": 2.0 ** 15}           # the dtype's upper admission bound on tau
ROOT_TAUS = ["lo", "1e-3", "one", "hi", "under", "over"]     # 2^-20, 1e-3, 1, the upper bound, 2^-21, twice the upper bound
QUOTIENT_TAUS = ["lo", "1e-3", "one", "hi"]
MIN_COMPARED = {"f16": 31744, "bf16": 32640}            # the non-negative finite patterns
OTHER_HYPER = dict(beta_1=0.5, beta_2=1.25, eta=4.0, tau=1024.0)     # test_gpu_f16_chain_edges.py's


def _tau(dt, name):
    return {"lo": 2.0 ** -20, "1e-3": 1e-3, "one": 1.0, "hi": UPPER[dt], "under": 2.0 ** -21,
            "over": 2 * UPPER[dt]}[name]


@functools.lru_cache(maxsize=1)
def _source(kind, dt):
    return {"root": F.root_source, "quotient": F.quotient_source, "moment": F.moment_source}[kind](DTYPES[dt])


@functools.lru_cache(maxsize=1)
def _expected_cached(kind, dt, sort, hyper):
    src = _source(kind, dt)
    if kind == "moment":
        exp = F.oracle_step(sort, dict(hyper), torch.zeros(src.n + 2, dtype=src.dtype), src.m, src.v, src.client)
    else:
        exp = F.oracle_collapsed(sort, hyper, src)
    return tuple(t.to(DEV) for t in exp)


def _expected(kind, dt, sort, hyper):
    """The oracle's (current', m', v') on the sweep's source, on the device; computed when the sweep,
    dtype, variant or hyperparameters change (the cases are ordered so that they change last)."""
    from oracle import consult
    consult.note()      # every case compares with the oracle's results, whichever case computed them
    return _expected_cached(kind, dt, sort, hyper)


def _cases(taus, packings):
    return [pytest.param(*c, id="-".join(c)) for c in
            itertools.product(DTYPES, F.SORTS, taus, packings, F.LAYOUTS, F.KERNELS)]


@pytest.mark.parametrize("dt,sort,tau,packing,layout,kernel", _cases(ROOT_TAUS, F.PACKINGS))
def test_root_sweep(dt, sort, tau, packing, layout, kernel):
    """current' = RN(m / RN(RN(sqrt(v)) + tau)) on every v.  At the two taus outside [2^-20, upper]
    the whole tensor takes the general path and still matches."""
    t = _tau(dt, tau)
    src = _source("root", dt)
    masks = F.run_case(f"root/{dt}/{sort}", sort, F.collapse_hyper(sort, t), kernel, layout, packing, src,
                       _expected("root", dt, sort, t), DEV)
    n = int(masks["current"].sum())
    print(f"root/{dt}/{sort}/tau={t}/{packing}/{layout}/{kernel}: {n} of {src.n} compared bitwise")
    assert n >= MIN_COMPARED[dt], n
    assert int(masks["v"].sum()) >= 2 * MIN_COMPARED[dt] and bool(masks["m"].all())


@pytest.mark.parametrize("dt,sort,tau,packing,layout,kernel", _cases(QUOTIENT_TAUS, F.PACKINGS))
def test_quotient_sweep(dt, sort, tau, packing, layout, kernel):
    """current' = RN(m / den) on every m x the v list: den spans [tau, sqrt(v_max) + tau]."""
    t = _tau(dt, tau)
    src = _source("quotient", dt)
    masks = F.run_case(f"quotient/{dt}/{sort}", sort, F.collapse_hyper(sort, t), kernel, layout, packing, src,
                       _expected("quotient", dt, sort, t), DEV)
    m, v = src.m[:src.n], src.v[:src.n]
    required = ~torch.isnan(m) & ~torch.signbit(v)          # every pair whose m is not NaN (no v is negative)
    n = int(masks["current"].sum())
    print(f"quotient/{dt}/{sort}/tau={t}/{packing}/{layout}/{kernel}: {n} of {src.n} compared bitwise, "
          f"{int(required.sum())} required")
    assert bool(required.any()) and bool(masks["current"][required].all())
    assert bool(masks["m"][required].all()) and bool(masks["v"].all())


@pytest.mark.parametrize("dt,sort,hyper,layout,kernel", [
    pytest.param(*c, id="-".join(c)) for c in
    itertools.product(DTYPES, F.SORTS, ["default", "other"], F.LAYOUTS, F.KERNELS)])
def test_moment_sweep(dt, sort, hyper, layout, kernel):
    """d = every bit pattern x 64 (m, v) states through the whole step: d * d overflowing, FedYogi's
    sign on every sign, zero and NaN of v - d^2, the packed fp16 ops and the scalar products on every
    half.  The pure packing: the lanes mix paths on their own here."""
    h = tuple(sorted(OTHER_HYPER.items())) if hyper == "other" else ()
    src = _source("moment", dt)
    masks = F.run_case(f"moment/{dt}/{sort}/{hyper}", sort, dict(h), kernel, layout, "pure", src,
                       _expected("moment", dt, sort, h), DEV)
    counts = {k: int(v.sum()) for k, v in masks.items()}
    print(f"moment/{dt}/{sort}/{hyper}/{layout}/{kernel}: compared bitwise {counts} of {src.n}")
    # m' = RN(RN(beta_1 m) + RN((1 - beta_1) d)) is a number wherever m and d are finite (|beta_1| and
    # |1 - beta_1| are below 1: neither product overflows): all of those were compared bitwise
    finite = torch.isfinite(src.m[:src.n]) & torch.isfinite(src.client[:src.n])
    assert int(finite.sum()) > src.n // 2 and bool(masks["m"][finite].all())
