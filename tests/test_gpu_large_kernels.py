"""Maximum sizes for the kernels that came after tests/test_gpu_large.py: each one on a key whose
element index crosses 2^31 -- and, for 1- and 2-byte elements, 2^32, where an index evaluated in
``unsigned`` wraps (tests/large_case.py: ``P16 = 2^32 + 70,001``, ``P32 = 2^31 + 4,099``).

Sampled cases compare bitwise at ``large_case.index(P)``: the boundaries, every element at or past
2^32, 20,000 random indices.  Their inputs come from the counter generator on the device; the
reference reads the host restatement of it, and each case first asserts that the device tensor holds
those bits (``case_dev`` / ``pinned``), which pins flame_synth_fill past 2^32 as well.  Reductions
along an update (statistics, distances, Gram) cannot be sampled: their inputs are small integers, so
every fp64 sum is the exact integer in any order, and sentinels at the 32-bit boundaries make a
missed or doubled read show.  Every case asserts the names of the native launches it made.
tests/test_large_case_host.py shows on the CPU that a wrapped index would change these references.

One test per kernel; each states its bytes in its leading ``_need`` and frees them at its end.
"""
import copy

import numpy as np
import pytest
import torch

import large_case as LC
import noise_ref as NR
import scenarios as S
import select_ref as SR
import trimmed_ref as R
import uplink16_case as U
from large_case import DEV, P16, P32, Launches, _at, _free, _need

pytestmark = [pytest.mark.gpu]
oracle = pytest.mark.oracle

BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
GB16 = P16 * 2 / 1e9            # one 2-byte tensor of P16 elements
GB32 = P32 * 4 / 1e9            # one fp32 tensor of P32 elements: the same bytes
_IDX = {}


def _index(P):
    if P not in _IDX:
        _IDX[P] = LC.index(P)
    return _IDX[P]


def _make(sort, **kw):
    from flame_amd.optimizers import optimizer_provider
    return optimizer_provider.get(sort, **kw)


# ---------------------------------------------------------------------------- 1-3: the reductions
@oracle
def test_reduce_scaled_past_2_32_elements():
    """flame_agg_reduce_scaled: two clipped bf16 clients into a bf16 aggregate."""
    from oracle import oracle as O
    from flame_amd import engine
    _need(3 * GB16 + 2)
    idx = _index(P16)
    base, ups, b_s, u_s = LC.case_dev(P16, LC.SEED["scaled"], idx, 2, 1.0, BF16, BF16)
    scales = [0.37, 1.0]
    with Launches() as ln:
        engine.accumulate({"w": base}, [({"w": u}, r) for u, r in zip(ups, LC.RATES)], scales=scales)
    torch.cuda.synchronize()
    assert ln.names == ["flame_agg_reduce_scaled"], ln.names
    exp = b_s.clone()
    O.reduce_tensor(exp, [O.tmp_tensor(u, s) for u, s in zip(u_s, scales)], LC.RATES)
    S.assert_bitwise("scaled", {"w": _at(base, idx)}, {"w": exp})
    del base, ups
    _free()


def test_reduce_mixed_past_2_32_elements():
    """flame_agg_reduce_mixed: two bf16 clients into an fp32 aggregate (2-byte and 4-byte strides)."""
    from flame_amd import engine
    _need(4 * GB16 + 2)
    idx = _index(P16)
    base, ups, b_s, u_s = LC.case_dev(P16, LC.SEED["mixed"], idx, 2, 1.0, F32, BF16)
    with Launches() as ln:
        engine.accumulate({"w": base}, [({"w": u}, r) for u, r in zip(ups, LC.RATES)])
    torch.cuda.synchronize()
    assert ln.names == ["flame_agg_reduce_mixed"], ln.names
    S.assert_bitwise("mixed", {"w": _at(base, idx)}, {"w": U.restate(b_s, u_s, LC.RATES)})
    del base, ups
    _free()


def _bytes_at(t, idx):
    """``t`` (uint8, on the device) at ``idx`` by index_select -- and, for the part at or past 2^32, by
    a contiguous slice as well: these inputs have no host restatement, so the sampler itself is
    checked where a wrapped sampler would make the comparison vacuous."""
    got = _at(t, idx)
    past = idx >= 1 << 32
    if bool(past.any()):
        lo = int(idx[past][0])
        assert torch.equal(got[past], t[lo:].cpu()[idx[past] - lo])
    return got


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
def test_reduce_mx_past_2_32_elements(fmt):
    """flame_agg_reduce_mx: two MX clients of random element bytes (every NaN byte among them) and
    scale bytes 2^-8 .. 2^8 into an fp32 aggregate; the scale byte of element e is at e / 32."""
    from flame_amd import engine, mx
    _need(2 * GB16 + 2 * P16 / 1e9 + 3)
    idx = _index(P16)
    dt = mx.FORMATS[fmt][0]
    seed = LC.SEED["mx"]
    b_s = LC.host_synth(seed, 0, idx, 1.0)
    base = LC._synth(P16, seed, 0, 1.0)
    LC.pinned("mx base", base, idx, b_s)
    g = torch.Generator(device=DEV).manual_seed(seed)
    nb = mx.n_blocks(P16)
    qs = [torch.randint(0, 256, (P16,), dtype=torch.uint8, device=DEV, generator=g) for _ in range(2)]
    ss = [torch.randint(119, 136, (nb,), dtype=torch.uint8, device=DEV, generator=g) for _ in range(2)]
    deq = []
    for q, s in zip(qs, ss):
        # mx.dequantize over blocks that hold the sample in their first element
        blocks = torch.zeros(idx.numel(), mx.BLOCK, dtype=torch.uint8)
        blocks[:, 0] = _bytes_at(q, idx)
        w = mx.MXWeights({"w": blocks.view(-1).view(dt)}, {"w": _bytes_at(s, idx // mx.BLOCK)})
        deq.append(mx.dequantize(w)["w"][::mx.BLOCK].contiguous())
    ws = [mx.MXWeights({"w": q.view(dt)}, {"w": s}) for q, s in zip(qs, ss)]
    with Launches() as ln:
        engine.accumulate({"w": base}, list(zip(ws, LC.RATES)))
    torch.cuda.synchronize()
    assert ln.names == ["flame_agg_reduce_mx"], ln.names
    S.same_bits(f"mx/{fmt}", {"w": _at(base, idx)}, {"w": U.restate(b_s, deq, LC.RATES)})
    del base, qs, ss, ws
    _free()


# ---------------------------------------------------------------------------- 4-5: the robust means
def _robust(row, entry, kernel, ref):
    _need(4 * GB16 + 2)
    idx = _index(P16)
    base, ups, b_s, u_s = LC.case_dev(P16, LC.SEED[row], idx, 3, LC.ROBUST_BASE_SIGMA, BF16, BF16)
    with Launches() as ln:
        entry({"w": base}, [{"w": u} for u in ups], 1)
    torch.cuda.synchronize()
    assert ln.names == [kernel], ln.names
    R.same_bits(row, _at(base, idx), ref(u_s, 1, b_s, BF16))
    del base, ups
    _free()


def test_trimmed_mean_past_2_32_elements():
    """flame_agg_trimmed: the median of 3 bf16 updates added to a base of their own magnitude."""
    from flame_amd import engine
    _robust("trimmed", engine.trimmed_mean, "flame_agg_trimmed", R.stream)


def test_selected_mean_past_2_32_elements():
    """flame_agg_select: the same round on the radix-select kernel."""
    from flame_amd import engine
    _robust("select", engine.selected_mean, "flame_agg_select", SR.select)


# ---------------------------------------------------------------------------- 6-8: reductions along an update
SLICE = 1 << 27


def _exact_dot(x, y, z=None):
    """sum((x - z) * (y - z)) with the non-finite elements of x and y taken out (zero, whatever z
    holds there), as a Python int: torch on the device in slices of 2^27 elements, each an exact
    fp64 dot product of small integers, added as Python ints."""
    def widened(t, lo):
        s = t[lo:lo + SLICE]
        d = s.double() if z is None else s.double() - z[lo:lo + SLICE].double()
        return torch.where(torch.isfinite(s), d, torch.zeros_like(d))
    total = 0
    for lo in range(0, x.numel(), SLICE):
        a = widened(x, lo)
        v = float(torch.dot(a, a if y is x else widened(y, lo)))
        assert v == int(v)
        total += int(v)
    return total


def _integer_updates(idx):
    """The three updates of rows 6-8: dense small integers, the six sentinels over zeros, and NaN /
    +inf / -inf at the sentinels' positions over zeros."""
    seed = LC.SEED["stats"]
    dense = LC._synth(P16, seed, 1, LC.DENSE_SIGMA, BF16)
    raw = LC.pinned("dense", dense, idx, LC.host_synth(seed, 1, idx, LC.DENSE_SIGMA, BF16))
    LC.integer_valued(dense)
    assert torch.equal(_at(dense, idx), LC.integer_valued(raw.clone()))
    sparse = torch.zeros(P16, dtype=BF16, device=DEV)
    bad = torch.zeros(P16, dtype=BF16, device=DEV)
    specials = [float("nan"), float("inf"), float("-inf")]
    for j, p in enumerate(LC.sentinels(P16)):
        sparse[p:p + 1].fill_(LC.SENTINEL_VALUES[j])      # a slice: host pointer arithmetic, no index kernel
        bad[p:p + 1].fill_(specials[j % 3])
    return [dense, sparse, bad]


SUMSQ_SENTINELS = sum(4 ** j for j in range(6))


@pytest.mark.parametrize("placement", ["tensors", "slab"])
def test_update_stats_past_2_32_elements(placement):
    """flame_update_stats: sumsq exact -- the dense update's against torch, the sentinels' sum(4**j),
    the non-finite update's 0 with a count of 6 -- from plain tensors and from tiled slab slots."""
    from flame_amd import engine
    from flame_amd.slab import UpdateSlab
    _need((6 if placement == "slab" else 3) * GB16 + 4)
    idx = _index(P16)
    ups = _integer_updates(idx)
    want = [_exact_dot(u, u) for u in ups]
    assert want[1] == SUMSQ_SENTINELS and want[2] == 0 and 8.5 * P16 < want[0] < 9.5 * P16
    ws = [{"w": u} for u in ups]
    if placement == "slab":
        slab = UpdateSlab({"w": torch.empty(P16, dtype=BF16, device="meta")}, capacity=3, device=DEV)
        d_s = _at(ups[0], idx)
        ws = [slab.put({"w": u}) for u in ups]
        del ups
        _free()
        assert torch.equal(_at(slab.read(ws[0].slot, "w"), idx), d_s)
    with Launches() as ln:
        sumsq, nf = engine.update_stats(ws, DEV)
    assert ln.names == ["flame_update_stats"], ln.names
    print(f"sumsq {[float(s) for s in sumsq]} want {want}; nonfinite {nf.tolist()}")
    assert [float(s) for s in sumsq] == [float(w) for w in want], (sumsq, want)
    assert nf.tolist() == [0, 0, 6]
    ups = ws = None
    _free()


def test_update_dist_past_2_32_elements():
    """flame_update_dist: the squared distances to an integer-valued centre, exact."""
    from flame_amd import engine
    _need(4 * GB16 + 4)
    idx = _index(P16)
    ups = _integer_updates(idx)
    seed = LC.SEED["stats"]
    z = LC._synth(P16, seed, 7, LC.DENSE_SIGMA, BF16)
    LC.pinned("centre", z, idx, LC.host_synth(seed, 7, idx, LC.DENSE_SIGMA, BF16))
    LC.integer_valued(z)
    want = [_exact_dot(u, u, z) for u in ups]
    with Launches() as ln:
        d2, nf = engine.update_dist([{"w": u} for u in ups], {"w": z}, DEV)
    assert ln.names == ["flame_update_dist"], ln.names
    print(f"dist2 {[float(s) for s in d2]} want {want}; nonfinite {nf.tolist()}")
    assert [float(s) for s in d2] == [float(w) for w in want], (d2, want)
    assert nf.tolist() == [0, 0, 6]
    del ups, z
    _free()


def test_update_gram_past_2_32_elements():
    """flame_update_gram: the exact 3 x 3 Gram matrix of the sanitised updates, both triangles."""
    from flame_amd import engine
    _need(3 * GB16 + 4)
    idx = _index(P16)
    ups = _integer_updates(idx)
    want = np.zeros((3, 3))
    for i in range(3):
        for j in range(i, 3):
            want[i, j] = want[j, i] = _exact_dot(ups[i], ups[j])
    assert want[1, 1] == SUMSQ_SENTINELS and not want[2].any()
    with Launches() as ln:
        gram, nf = engine.update_gram([{"w": u} for u in ups], DEV)
    assert ln.names == ["flame_update_gram"], ln.names
    print(f"gram {gram.tolist()} want {want.tolist()}; nonfinite {nf.tolist()}")
    assert np.array_equal(gram, want), (gram, want)
    assert nf.tolist() == [0, 0, 6]
    del ups
    _free()


# ---------------------------------------------------------------------------- 9-11
def _windows(P):
    """Starts of 8-element windows: one over every boundary of the sample set and the end, 64 random."""
    at = {min(max(b - 4, 0), P - 8) for b in LC.boundaries(P) + [P]}
    return sorted(at | set(np.random.default_rng(9).integers(0, P - 8, 64).tolist()))


@pytest.mark.parametrize("start", [0, 2 ** 33 + 1], ids=["vector", "element"])
def test_noise_fill_past_2_32_elements(start):
    """flame_noise_fill into one bf16 key: start 0 takes the vector path, an odd start past 2^33 the
    element path (its Philox blocks straddle the lanes' vectors)."""
    from flame_amd import engine
    _need(GB16 + 2)
    seed, rnd, stream, std = 0x1234_5678_9ABC, 3, 5, 0.75
    t = torch.empty(P16, dtype=BF16, device=DEV)
    with Launches() as ln:
        engine.noise_fill_([t], [stream], [start], seed, rnd, std)
    torch.cuda.synchronize()
    assert ln.names == ["flame_noise_fill"], ln.names
    wins = _windows(P16)
    widx = torch.from_numpy(np.concatenate([np.arange(w, w + 8) for w in wins]).astype(np.int64))
    got = _at(t, widx).view(torch.int16).numpy().view(np.uint16)
    want = np.concatenate([NR.fill("bf16", seed, rnd, stream, start + w, 8, std) for w in wins])
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} of {got.size} differ, first at element {int(widx[bad[0]])}"
    del t
    _free()


@oracle
def test_scale_add_past_2_32_elements():
    """flame_fedbuff_scale_add (the stand-alone kernel) with deltas, goal 3."""
    from oracle import oracle as O
    from flame_amd import engine
    _need(3 * GB16 + 2)
    idx = _index(P16)
    base, (agg,), b_s, (a_s,) = LC.case_dev(P16, LC.SEED["scale_add"], idx, 1, 1.0, BF16, BF16)
    delta = torch.empty_like(base)
    with Launches() as ln:
        engine.scale_add_([base], [agg], 3, deltas=[delta])
    torch.cuda.synchronize()
    assert ln.names == ["flame_fedbuff_scale_add"], ln.names
    ow = b_s.clone()
    od = O.scale_add_tensor(ow, a_s, 3, want_delta=True)
    S.assert_bitwise("scale_add/w", {"w": _at(base, idx)}, {"w": ow})
    S.assert_bitwise("scale_add/delta", {"w": _at(delta, idx)}, {"w": od})
    del base, agg, delta
    _free()


@oracle
def test_elementwise_past_2_32_elements():
    """flame_elementwise: bf16 updates into an f16 model, the promoted route of FedAvg (a grid-stride
    loop under a capped grid) -- not the uplink kernel, which takes fp32 models only."""
    from oracle import oracle as O
    _need(3 * GB16 + 2)
    idx = _index(P16)
    base, ups, b_s, u_s = LC.case_dev(P16, LC.SEED["elementwise"], idx, 2, 1.0, F16, BF16)
    counts = [3, 5]
    cache, ocache = S.SortedCache(), S.SortedCache()
    for i in range(2):
        cache[f"{i}"] = S.TR({"w": ups[i]}, counts[i])
        ocache[f"{i}"] = S.TR({"w": u_s[i]}, counts[i])
    with Launches() as ln:
        out = _make("fedavg").do({"w": base}, cache, total=sum(counts))
    torch.cuda.synchronize()
    assert ln.elementwise() >= 1 and ln.elementwise() == len(ln.names), ln.names
    assert ln.count("flame_agg_reduce_mixed") == 0
    exp = O.OracleFedAvg().do({"w": b_s.clone()}, ocache, total=sum(counts))
    S.assert_bitwise("elementwise", {"w": _at(out["w"], idx)}, exp)
    del out, base, ups, cache
    _free()


# ---------------------------------------------------------------------------- 12-14: fp32 / fp64 state
@oracle
def test_feddyn_round_past_2_31_elements():
    """flame_feddyn_round: FedDyn.do, two trainers, one round from empty histories -- the average,
    cld_model and both new histories bitwise against the oracle."""
    from oracle import oracle as O
    _need(6 * GB32 + 2)
    idx = _index(P32)
    base, ups, b_s, u_s = LC.case_dev(P32, LC.SEED["feddyn"], idx, 2, 1.0, F32, F32)
    ends, counts = ["e0", "e1"], [7, 8]
    amd, ora = _make("feddyn", alpha=0.01, history="rows"), O.OracleFedDyn(alpha=0.01)
    amd.save_state(S._PRE, active_ends=ends)
    ora.save_state(S._PRE, active_ends=ends)
    cache, ocache = S.SortedCache(), S.SortedCache()
    for e, u, us, c in zip(ends, ups, u_s, counts):
        cache[e] = S.TR({"w": u}, c)
        ocache[e] = S.TR({"w": us.clone()}, c)
    with Launches() as ln:
        a = amd.do({"w": base}, cache, total=sum(counts))
    torch.cuda.synchronize()
    assert ln.names == ["flame_feddyn_round"], ln.names
    o = ora.do({"w": b_s.clone()}, ocache, total=sum(counts))
    S.assert_bitwise("feddyn/avg", {"w": _at(a["w"], idx)}, o)
    S.assert_bitwise("feddyn/cld", {"w": _at(amd.cld_model["w"], idx)}, ora.cld_model)
    assert list(amd.local_param_dict) == list(ora.local_param_dict) == ends
    for e in ends:
        S.assert_bitwise(f"feddyn/hist/{e}", {"w": _at(amd.local_param_dict[e]["w"], idx)}, ora.local_param_dict[e])
    del a, base, ups, cache, amd
    _free()


@oracle
def test_fedopt_chain_past_2_31_elements():
    """flame_fedopt_chain: FedAdam(defer=True), two eager rounds of two arrivals, one launch per round;
    the FedAvg part (the base) bitwise, current / m_t / v_t within the SURVEY §8(c) contract
    (elementwise in the first round, rel-L2 after), as tests/test_gpu_eager_fedopt_chain.py holds it."""
    from oracle import oracle as O
    _need(9 * GB32 + 2)
    idx = _index(P32)
    seed, counts = LC.SEED["chain"], [4, 9]
    opt, ora = _make("fedadam", defer=True), O.OracleFedOPT("fedadam")
    w_s = LC.host_synth(seed, 0, idx, 1.0)
    w = LC._synth(P32, seed, 0, 1.0)
    LC.pinned("chain model", w, idx, w_s)
    weights, oweights = {"w": w}, {"w": w_s}
    del w
    for r in range(2):
        base = {k: v.clone() for k, v in dict(weights).items()}
        obase = copy.deepcopy(oweights)
        ups, u_s = [], []
        for i in range(2):
            u_s.append(LC.host_synth(seed, 10 * (r + 1) + i, idx, LC.UP_SIGMA))
            ups.append(LC._synth(P32, seed, 10 * (r + 1) + i, LC.UP_SIGMA))
            LC.pinned(f"chain r{r} update {i}", ups[i], idx, u_s[i])
        cache, ocache, total = S.SortedCache(), S.SortedCache(), 0
        with Launches() as ln:
            for i in range(2):
                total += counts[i]
                cache[f"r{r}e{i}"] = S.TR({"w": ups[i]}, counts[i])
                ocache[f"r{r}e{i}"] = S.TR({"w": u_s[i].clone()}, counts[i])
                out = opt.do(base, cache, total=total, num_trainers=2)
                oout = ora.do(obase, ocache, total=total)
            weights, oweights = out, oout
            cur = dict(out)                     # the read runs the queue; the base is final after it
            torch.cuda.synchronize()
        assert ln.count("flame_fedopt_chain") == 1 and ln.count("flame_fedopt_reduce_adapt") == 0, ln.names
        assert ln.elementwise() == 0, ln.names
        S.assert_bitwise(f"chain/r{r}/base", {"w": _at(base["w"], idx)}, obase)
        S.assert_close_fedopt(f"chain/r{r}/current", {"w": _at(cur["w"], idx)}, oout, elementwise=r == 0)
        S.assert_close_fedopt(f"chain/r{r}/m", {"w": _at(opt.m_t["w"], idx)}, ora.m_t, elementwise=r == 0)
        S.assert_close_fedopt(f"chain/r{r}/v", {"w": _at(opt.v_t["w"], idx)}, ora.v_t, elementwise=r == 0)
        del ups, cache, base, cur, out
        _free()
    del weights, opt
    _free()


@oracle
def test_fedadam_f64_past_2_31_elements():
    """flame_fedopt_reduce_adapt_f64: FedAdam on an fp64 key, one client, the passthrough round and
    the zero-state adaptive round, bitwise against OracleFedOPT(sqrt_rn=True)."""
    from oracle import oracle as O
    from flame_amd import _native
    _need(6 * P32 * 8 / 1e9 + 4)
    idx = _index(P32)
    seed = LC.SEED["f64"]
    opt, ora = _make("fedadam"), O.OracleFedOPT("fedadam", sqrt_rn=True)
    ocur = LC.host_synth(seed, 0, idx, 1.0, F64)
    cur = LC._synth(P32, seed, 0, 1.0, F64)
    LC.pinned("f64 model", cur, idx, ocur)
    branch = "flame_fedopt_reduce_adapt/f64/fedadam"
    for r in range(2):
        u_s = LC.host_synth(seed, 10 * (r + 1), idx, LC.UP_SIGMA, F64)
        up = LC._synth(P32, seed, 10 * (r + 1), LC.UP_SIGMA, F64)
        LC.pinned(f"f64 r{r} update", up, idx, u_s)
        c, oc = S.SortedCache(), S.SortedCache()
        c["0"] = S.TR({"w": up}, 4)
        oc["0"] = S.TR({"w": u_s}, 4)
        before = _native.launch_branch_counts().get(branch, 0)
        with Launches() as ln:
            # the caller's do(deepcopy(self.weights), ...) (syncfl/top_aggregator.py:161-166)
            cur = opt.do({"w": cur.clone()}, c, total=4)["w"]
        torch.cuda.synchronize()
        ocur = ora.do({"w": ocur.clone()}, oc, total=4)["w"]
        del up, c
        _free()
        fused = _native.launch_branch_counts().get(branch, 0) - before
        assert fused == r and ln.count("flame_fedopt_reduce_adapt") == r and ln.elementwise() == 0, (r, fused, ln.names)
        assert cur.dtype == F64
        S.same_bits(f"f64/r{r}/avg", {"w": _at(opt.agg_weights["w"], idx)}, ora.agg_weights)
        S.same_bits(f"f64/r{r}/cur", {"w": _at(cur, idx)}, {"w": ocur})
        if r == 1:
            S.same_bits("f64/r1/m", {"w": _at(opt.m_t["w"], idx)}, ora.m_t)
            S.same_bits("f64/r1/v", {"w": _at(opt.v_t["w"], idx)}, ora.v_t)
    del cur, opt
    _free()
