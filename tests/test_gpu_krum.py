"""GPU: Krum / Multi-Krum -- flame_update_gram (fp64 matrix cores), engine.update_gram and the
optimizers' ``krum`` / ``krum_select`` kwargs.

* Exact Gram: on integer-valued updates in [-8, 8] every product and every partial sum is exact in
  fp64 in any order, so ``G`` must be BITWISE the exact Gram matrix, both triangles -- the check with
  exact integer data that a matrix-core lane map needs.  Every client differs, so off-diagonal
  blocks are asymmetric and a swapped or mis-rowed C/D map shows.
* Ordinary data: each ``G[i][j]`` against ``math.fsum`` of the fp64 products (correctly rounded),
  ``|err| <= (n_el + 1) * 2^-53 * sum |x_i x_j|`` for f32 / bf16 / f16 (their products are exact in
  fp64; Higham's bound for a sum of n_el terms in any order, plus the reference's own rounding) and
  ``(n_el + 2) * 2^-53`` for f64 (one more rounding per product, which an fma and the reference's
  multiply may place differently).  Derived, not measured; the measured maxima are printed.
* Optimizers: the selected ends equal tests/krum_ref.py's (distances formed directly, never through a
  Gram matrix), and the model is bitwise the oracle's FedAvg statement over the selected updates in
  cache order with rate 1 / m (FedAdam: the oracle's FedOPT step on that average).

Every optimizer test consults the CPU oracle, so the branches they reach are credited.
"""
import fractions
import itertools
import math

import numpy as np
import pytest
import torch

import krum_ref as R
import scenarios as S

pytestmark = [pytest.mark.gpu, pytest.mark.oracle]

DEV = "cuda:0"
U53 = 2.0 ** -53
SIZES = [1023, 0, 1, 3, 1024, 4099]      # several keys per model, an empty one among them
BIG = 300_001
DTYPES = [torch.float32, torch.bfloat16, torch.float16, torch.float64]
IDS = ["f32", "bf16", "f16", "f64"]
LAYOUTS = ["tensors", "slab", "misaligned"]
NS = [1, 2, 15, 16, 17, 33, 64, 65, 130]   # block edges (16), tile edges (64), a ragged third tile


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    from flame_amd import _native
    _native.lib()
    assert torch.cuda.is_available()


def _oracle():
    from oracle import oracle as O
    return O


def _drop_in(sort, **kw):
    from flame_amd.optimizers import optimizer_provider
    return optimizer_provider.get(sort, **kw)


def _layout(ups, layout):
    """The same updates on the GPU as plain tensors, UpdateSlab slots (tiled), or views one element
    off 16-byte alignment (the bounded element loads)."""
    if layout == "tensors":
        return [S.to_dev(w, DEV) for w in ups], None
    if layout == "misaligned":
        out = []
        for w in ups:
            d = {}
            for k, v in w.items():
                buf = torch.empty(v.numel() + 1, dtype=v.dtype, device=DEV)
                buf[1:].copy_(v.reshape(-1))
                d[k] = buf[1:].view(v.shape)
                assert v.numel() == 0 or d[k].data_ptr() % 16 != 0
            out.append(d)
        return out, None
    from flame_amd.slab import UpdateSlab
    slab = UpdateSlab(ups[0], len(ups), DEV)
    return [slab.put(S.to_dev(w, DEV)) for w in ups], slab


def _fill(ups, counts=None):
    cache = S.SortedCache()
    for i, u in enumerate(ups):
        cache[f"e{i:04d}"] = S.TR(u, 1 if counts is None else counts[i])
    return cache


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class _Launches:
    """Names of the native launches made inside the block (engine._recorders)."""

    def __enter__(self):
        from flame_amd import engine
        self.events = []
        engine._recorders.append(self.events)
        return self

    def __exit__(self, *exc):
        from flame_amd import engine
        engine._recorders.remove(self.events)
        self.names = [ev[0] for ev in self.events]
        return False

    def count(self, name):
        return sum(1 for n in self.names if n == name)


def _check_average(label, ws, ups, sel):
    """The round's last step on these very device updates: the updates ``sel`` through the existing
    reduction (engine.accumulate) with rate 1 / len(sel), bitwise the oracle's reduce_tensor."""
    from flame_amd import engine
    O = _oracle()
    rates = [1.0 / len(sel)] * len(sel)
    agg = {k: torch.zeros(v.shape, dtype=v.dtype, device=DEV) for k, v in ups[0].items()}
    engine.accumulate(agg, [(ws[i], rates[0]) for i in sel], device=torch.device(DEV))
    exp = {k: torch.zeros(v.shape, dtype=v.dtype) for k, v in ups[0].items()}
    for k in exp:
        O.reduce_tensor(exp[k], [ups[i][k] for i in sel], rates)
    S.same_bits(label, agg, exp)


def _selected(gram, nf, f):
    from flame_amd.optimizer import krum
    return krum.select(gram, nf, None, f, len(nf) - f)[1]


# ---------------------------------------------------------------------------- 1. exact Gram
_INT = {}


def _int_bank(n, big):
    """``n`` integer-valued fp64 updates over SIZES (+ the 300,001-element key) and their exact Gram
    matrix: generated once, shared by every dtype and layout, never modified."""
    key = (n, big)
    if key not in _INT:
        g = torch.Generator().manual_seed(500 + n)
        ups = R.integer_updates(g, n, SIZES + ([BIG] if big else []), torch.float64)
        _INT[key] = (ups, R.exact_gram(ups))
    return _INT[key]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_exact_gram_bitwise(dt, layout):
    """n in NS over six keys (6,150 elements: 9 fp32 chunks, so three chunk ranges of
    kGramMinR = 4 chunks per tile pair); for n = 17 and n = 130 one more key of 300,001 elements
    (293 fp32 / 147 16-bit / 586 fp64 chunks).  A workgroup's chunk range is
    max(4, ceil(n_chunks * pairs / 2048)) chunks, which is 4 at these shapes (pairs = 1 for
    n = 17, 6 for n = 130): MORE THAN ONE chunk range per tile pair is produced in every case (at
    least 37 with the large key), so the finish kernel's ordered sum over ranges is exercised, and
    n = 130 has a ragged third tile whose pairs with the first two are off-diagonal."""
    from flame_amd import engine
    for n in NS:
        ups64, exact = _int_bank(n, n in (17, 130))
        ups = [{k: v.to(dt) for k, v in u.items()} for u in ups64]
        ws, slab = _layout(ups, layout)
        gram, nf = engine.update_gram(ws, DEV)
        label = f"{IDS[DTYPES.index(dt)]}/{layout}/n{n}"
        assert gram.dtype == np.float64 and gram.shape == (n, n) and nf.dtype == np.int64 and nf.shape == (n,), label
        bad = np.argwhere(_bits(gram) != _bits(exact))
        assert bad.size == 0, f"{label}: {len(bad)} entries differ, first {bad[:4].tolist()}: " \
                              f"{[(gram[i, j], exact[i, j]) for i, j in bad[:4]]}"
        assert np.array_equal(_bits(gram), _bits(gram.T)), label
        assert not nf.any(), label
        again, nf2 = engine.update_gram(ws, DEV)
        assert np.array_equal(_bits(gram), _bits(again)) and np.array_equal(nf, nf2), label
        if n == 17:         # ... and the selection's average over these updates, against the oracle
            sel = _selected(gram, nf, 4)
            assert sel == R.select(R.distances(ups)[0], 4)[1] and len(sel) == 13
            _check_average(label, ws, ups, sel)
        del ws, slab


# ---------------------------------------------------------------------------- 2. the bound
_ORD = {}


def _ordinary(dt, n):
    """N(0, 1) * (0.5 + 0.01 i) in ``dt`` over SIZES, with fsum(x_i x_j) and sum |x_i x_j| per pair."""
    key = (dt, n)
    if key not in _ORD:
        g = torch.Generator().manual_seed(100 + DTYPES.index(dt))
        ups = [{f"k{j}": (torch.randn(s, generator=g) * (0.5 + 0.01 * i)).to(dt) for j, s in enumerate(SIZES)}
               for i in range(n)]
        flat = [R.flatten(u)[0] for u in ups]
        ref, mag = np.empty((n, n)), np.empty((n, n))
        for i in range(n):
            for j in range(i, n):
                p = flat[i] * flat[j]             # exact for f32 / bf16 / f16 inputs; one rounding for f64
                ref[i, j] = ref[j, i] = math.fsum(p)
                mag[i, j] = mag[j, i] = math.fsum(np.abs(p))
        _ORD[key] = (ups, ref, mag)
    return _ORD[key]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_gram_within_the_any_order_bound(dt, layout):
    from flame_amd import engine
    n_el = sum(SIZES)
    for n in (9, 65):
        ups, ref, mag = _ordinary(dt, n)
        ws, slab = _layout(ups, layout)
        gram, nf = engine.update_gram(ws, DEV)
        tol = (n_el + (2 if dt == torch.float64 else 1)) * U53
        ratio = np.abs(gram - ref) / mag
        print(f"{IDS[DTYPES.index(dt)]}/{layout}/n{n}: max |err| / sum|x_i x_j| = {ratio.max():.3e} (bound {tol:.3e})")
        assert (ratio <= tol).all(), f"{ratio.max():.3e} > {tol:.3e}"
        assert np.array_equal(_bits(gram), _bits(gram.T)) and not nf.any()
        # the diagonal is the guard's sum of squares up to summation order
        sumsq, nf_s = engine.update_stats(ws, DEV)
        assert (np.abs(sumsq - gram.diagonal()) <= 2 * tol * sumsq).all() and np.array_equal(nf, nf_s)
        if n == 9:
            _check_average(f"{layout}/n{n}", ws, ups, _selected(gram, nf, 2))
        del ws, slab


# ---------------------------------------------------------------------------- 3. special values
def _from_bits(pattern, dt):
    it = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16,
          torch.float64: torch.int64}[dt]
    return torch.tensor([pattern], dtype=torch.int64).to(it).view(dt)[0]


def _nans(dt):
    width = torch.empty((), dtype=dt).element_size() * 8
    mant = {torch.float32: 23, torch.bfloat16: 7, torch.float16: 10, torch.float64: 52}[dt]
    expo = ((1 << (width - 1 - mant)) - 1) << mant
    pos = expo | (1 << (mant - 1)) | 1
    neg = pos | (1 << (width - 1))
    if neg >= 1 << (width - 1):
        neg -= 1 << width                     # as a signed pattern
    p, m = _from_bits(pos, dt), _from_bits(neg, dt)
    assert bool(torch.isnan(p)) and bool(torch.isnan(m))
    return p, m


def _exact_sanitised_gram(ups):
    """The Gram matrix of the sanitised elements in rational arithmetic, rounded once to fp64
    (an overflow is +-inf)."""
    flat = [[fractions.Fraction(x) for x in R.flatten(u)[0].tolist()] for u in ups]
    n = len(flat)
    out = np.empty((n, n))
    for i in range(n):
        for j in range(i, n):
            v = sum((a * b for a, b in zip(flat[i], flat[j]) if a and b), fractions.Fraction(0))
            try:
                r = float(v)
            except OverflowError:
                r = math.inf if v > 0 else -math.inf
            out[i, j] = out[j, i] = r
    return out


@pytest.mark.parametrize("with_max", [False, True], ids=["no-max", "max"])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_special_values(dt, with_max):
    """NaN of both signs, +-inf, +-0 and subnormals of both signs planted in a whole aligned chunk
    (the vector loads) and in the tail chunk (the bounded loads), each at three coordinates where
    1, 2 and all 5 clients hold it -- the inf * 0 and NaN * NaN pairs.  Counts are exact and ``G`` is
    the exact Gram matrix of the sanitised data rounded once (integers in [-8, 8] elsewhere: a
    subnormal's products are far below half an ulp of the integer sums, so every order gives that
    rounding).  ``with_max``: +max at one coordinate and -max at another of EVERY client, so all
    their products have one sign and no order can cancel them; max^2 stays finite in fp64 for f32 /
    bf16 / f16 and overflows for f64, where the whole matrix is +inf (the ineligible case)."""
    from flame_amd import engine
    n = 5
    T = engine.chunk_elems(engine.dtype_code(dt))
    numel = 2 * T + 37
    fi = torch.finfo(dt)
    pnan, nnan = _nans(dt)
    f64 = torch.float64
    sp = [pnan, nnan, torch.tensor(math.inf, dtype=dt), torch.tensor(-math.inf, dtype=dt), torch.tensor(0.0, dtype=dt),
          torch.tensor(-0.0, dtype=dt), torch.tensor(fi.smallest_normal, dtype=f64).div(4).to(dt),
          torch.tensor(-fi.smallest_normal, dtype=f64).div(8).to(dt)]
    g = torch.Generator().manual_seed(70 + DTYPES.index(dt))
    xs = [torch.randint(-8, 9, (numel,), generator=g).to(dt) for _ in range(n)]
    for off in (5, T + 200, 2 * T + 3):                       # two vector chunks, then the tail chunk
        for k, v in enumerate(sp):
            for c, holders in enumerate((1, 2, n)):
                for u in range(holders):
                    xs[(k + u) % n][off + 3 * k + c] = v
    if with_max:
        for x in xs:
            x[T - 9], x[2 * T + 33] = fi.max, fi.min
    ups = [{"x": x} for x in xs]
    want_nf = [int((~torch.isfinite(x)).sum()) for x in xs]
    assert min(want_nf) > 0
    exact = _exact_sanitised_gram(ups)
    if with_max:
        assert np.isinf(exact).all() == (dt == torch.float64) and np.isfinite(exact).all() == (dt != torch.float64)
    for layout in LAYOUTS:
        ws, slab = _layout(ups, layout)
        gram, nf = engine.update_gram(ws, DEV)
        assert nf.tolist() == want_nf, layout
        assert np.array_equal(_bits(gram), _bits(exact)), (layout, gram, exact)
        assert _selected(gram, nf, 1) == []                   # every update holds a non-finite element: none eligible
        _check_average(f"special/{layout}", ws, ups, list(range(n)))      # "keep": NaN / inf where torch-CPU puts them
        del ws, slab


# ---------------------------------------------------------------------------- 4. two dtypes
def test_two_dtype_model_and_ignored_keys():
    """f32 and bf16 keys (two launches accumulate into one ``G``), an int64 0-dim key and a bool mask
    that take no part; as tensors and as slab slots of a DeviceUpdateCache."""
    from flame_amd import engine
    from flame_amd.ingest import DeviceUpdateCache
    g = torch.Generator().manual_seed(5)
    ups = []
    for i in range(9):
        ups.append({"a": torch.randint(-8, 9, (4099,), generator=g).float(), "nbt": torch.tensor(7 + i),
                    "b": torch.randint(-8, 9, (3 * 2048 + 5,), generator=g).bfloat16(),
                    "mask": torch.rand(33, generator=g) > 0.5, "c": torch.randint(-8, 9, (17, 3), generator=g).float()})
    exact = R.exact_gram(ups)
    with _Launches() as ln:
        gram, nf = engine.update_gram([S.to_dev(w, DEV) for w in ups], DEV)
    assert ln.count("flame_update_gram") == 2, ln.names
    assert np.array_equal(_bits(gram), _bits(exact)) and not nf.any()
    _check_average("two-dtype", [S.to_dev(w, DEV) for w in ups], ups, _selected(gram, nf, 2))
    cache = DeviceUpdateCache(device=DEV, placement="slab", capacity=9)
    for i, w in enumerate(ups):
        cache[f"e{i}"] = S.TR({k: v.clone() for k, v in w.items()}, 1)
    gram2, nf2 = engine.update_gram([cache[f"e{i}"].weights for i in range(9)], DEV)
    assert np.array_equal(_bits(gram2), _bits(exact)) and not nf2.any()
    with pytest.raises(ValueError, match="'b'"):              # a missing key is refused by name
        engine.update_gram([S.to_dev(w, DEV) for w in ups[:3]] + [{"a": ups[3]["a"].to(DEV), "c": ups[3]["c"].to(DEV)}], DEV)


# ---------------------------------------------------------------------------- 5. optimizers
def _score_tol(q, n_el, max_gii):
    return q * (4 * (n_el + 2) + 4) * U53 * max_gii


def _check_scores(label, recs, ref_scores, q, n_el, ups, scales=None):
    s = [1.0] * len(ups) if scales is None else scales
    max_gii = max(float(np.dot(v, v)) * sc * sc for (v, _), sc in zip((R.flatten(u) for u in ups), s))
    tol = _score_tol(q, n_el, max_gii)
    worst = 0.0
    for r, ref in zip(recs, ref_scores):
        if math.isinf(ref):
            assert math.isinf(r.score), (label, r)
            continue
        worst = max(worst, abs(r.score - ref))
        assert abs(r.score - ref) <= tol, (label, r, ref, tol)
    print(f"{label}: max |score - ref| = {worst:.3e} (bound {tol:.3e})")


def _model(gen, n, f, dt, ints):
    ups, honest = R.honest_bad(gen, n, f, (4099, 210), dt)
    if ints:
        for i, u in enumerate(ups):
            u["nbt"] = torch.tensor(100 + 37 * i)
    return ups, honest


@pytest.mark.parametrize("sort", ["fedavg", "fedprox", "fedadam"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16], ids=IDS[:3])
def test_krum_optimizers_three_rounds(sort, dt):
    """``krum=2`` over 3 rounds of 9 updates (7 honest, 2 bad, tests/krum_ref.py's honest_bad).

    Selection: the selected ends are the reference's, which are the honest ones.

    Scores: within ``q * (4 (n_el + 2) + 4) * 2^-53 * max_i G[i][i]`` of the reference's.  Each of
    the q distances is ``(a_i + a_j) - 2 G[i][j]``.  ``|G[i][j]| <= sum |x_i x_j| <= max G`` by
    Cauchy-Schwarz, so each of the three Gram entries is within ``(n_el + 2) * 2^-53 * max G`` of its
    exact value and they enter with weights 1, 1 and 2: ``4 (n_el + 2) * 2^-53 * max G``.  The
    formula adds three roundings (the scaled product, the sum, the difference) of values of the
    order of max G: the ``+ 4``.  ``math.fsum`` adds none, and the reference's own directly summed
    distance is far inside the first term's slack.

    Model: bitwise the oracle's FedAvg over the selected updates in cache order with counts 1 and
    total m (rate 1 / m); FedAdam: the oracle's FedOPT step on that average, each round from
    identical state, as the guarded-FedOPT test does."""
    O = _oracle()
    n, f = 9, 2
    q, m = n - f - 2, n - f
    g = torch.Generator().manual_seed(31 + DTYPES.index(dt))
    kw = {"mu": 0.1} if sort == "fedprox" else {}
    adam = sort == "fedadam"
    opt = _drop_in(sort, krum=f, **kw)
    ora = O.OracleFedOPT(sort, sqrt_rn=True) if adam else O.OracleFedAvg()
    base = {"k0": torch.randn(4099, generator=g).to(dt), "k1": torch.randn(210, generator=g).to(dt)}
    if not adam:
        base["nbt"] = torch.tensor(7)
    fkeys = ("k0", "k1")
    n_el = 4099 + 210
    dev_base, ora_base = S.to_dev(base, DEV), S.to_cpu(base)
    for rnd in range(3):
        ups, honest = _model(g, n, f, dt, not adam)
        counts = [5 + i for i in range(n)]                   # counts play no part
        with _Launches() as ln:
            got = opt.do(dev_base, _fill([S.to_dev(u, DEV) for u in ups], counts), total=sum(counts))
        assert ln.count("flame_update_gram") == 1 and ln.count("flame_update_stats") == 0, ln.names
        ref_scores, ref_sel, _, _ = R.krum(ups, f)
        recs = opt.krum_records
        label = f"{sort}/{IDS[DTYPES.index(dt)]}/r{rnd}"
        assert [r.end for r in recs] == [f"e{i:04d}" for i in range(n)]
        sel = [i for i, r in enumerate(recs) if r.selected]
        assert sel == ref_sel == honest, label
        _check_scores(label, recs, ref_scores, q, n_el, ups)
        assert opt.update_stats == []                        # no guard: nothing measured for it
        exp = ora.do(ora_base, _fill([S.to_cpu(ups[i]) for i in sel]), total=m)
        S.assert_bitwise(f"{label}/avg", {k: dev_base[k] for k in base}, {k: ora_base[k] for k in base})
        if adam and dt == torch.float32 and rnd > 0:
            S.assert_close_fedopt(label, {k: got[k] for k in fkeys}, {k: exp[k] for k in fkeys})
        elif adam and rnd > 0:
            S.assert_bitwise(f"{label}/cur", {k: got[k] for k in fkeys}, {k: exp[k] for k in fkeys})
        else:
            S.assert_bitwise(f"{label}/cur", {k: got[k] for k in base}, {k: exp[k] for k in base})
        if adam:
            dev_base = {k: v.clone() for k, v in got.items()}
            ora_base = S.to_cpu(got)
            ora.current_weights = S.to_cpu(got)
            if opt.m_t is not None:
                ora.m_t, ora.v_t = S.to_cpu(opt.m_t), S.to_cpu(opt.v_t)


def test_krum_select_one_takes_the_single_lowest_score():
    from flame_amd.optimizer import FedKrum
    O = _oracle()
    g = torch.Generator().manual_seed(77)
    ups, honest = _model(g, 9, 2, torch.float32, True)
    ref_scores, ref_sel, _, _ = R.krum(ups, 2, 1)
    assert ref_sel == [int(np.argmin(ref_scores))] and ref_sel[0] in honest
    base = {"k0": torch.randn(4099, generator=g), "k1": torch.randn(210, generator=g), "nbt": torch.tensor(7)}
    for opt in (_drop_in("fedavg", krum=2, krum_select=1), FedKrum(2)):
        dev = S.to_dev(base, DEV)
        out = opt.do(dev, _fill([S.to_dev(u, DEV) for u in ups]), total=9)
        assert out is dev and [i for i, r in enumerate(opt.krum_records) if r.selected] == ref_sel
        exp = S.to_cpu(base)
        O.OracleFedAvg().do(exp, _fill([S.to_cpu(ups[ref_sel[0]])]), total=1)
        S.assert_bitwise("krum_select=1", {k: dev[k] for k in base}, exp)


# ---------------------------------------------------------------------------- 6. the property
def test_two_arbitrary_updates_are_never_selected():
    """7 honest updates (g + 0.1 N(0, 1)) and 2 arbitrary ones -- all-NaN, +-1e30, a sign-flipped
    honest copy, an honest copy x 8 -- in all 16 combinations, ``krum=2``: every selected update is
    honest and every coordinate of the result (base 0) lies within the honest values' [min, max];
    plain FedAvg on the same inputs leaves it for every combination."""
    from flame_amd.optimizer import FedAvg
    O = _oracle()
    g = torch.Generator().manual_seed(9)
    P = 4099
    center = torch.randn(P, generator=g)
    honest = [center + 0.1 * torch.randn(P, generator=g) for _ in range(7)]
    lo, hi = torch.stack(honest).min(0).values, torch.stack(honest).max(0).values
    alt = torch.tensor([1e30, -1e30]).repeat(P // 2 + 1)[:P]
    bad = {"nan": torch.full((P,), float("nan")), "+-1e30": alt, "flip": -honest[3], "x8": 8.0 * honest[5]}

    def holds(out):
        out = out.cpu()
        return bool((~torch.isnan(out)).all()) and bool(((out >= lo) & (out <= hi)).all())

    for a, b in itertools.product(bad, bad):
        ups = honest[:2] + [bad[a]] + honest[2:6] + [bad[b]] + honest[6:]
        hon = [0, 1, 3, 4, 5, 6, 8]
        outs = {}
        for name, opt in (("krum", FedAvg(krum=2)), ("plain", FedAvg())):
            outs[name] = opt.do({"w": torch.zeros(P, device=DEV)}, _fill([{"w": u.to(DEV)} for u in ups]), total=9)["w"]
            if name == "krum":
                sel = [i for i, r in enumerate(opt.krum_records) if r.selected]
                assert sel == hon, (a, b, sel)
                assert all(math.isinf(r.score) for r in opt.krum_records if r.nonfinite), (a, b)
        assert holds(outs["krum"]), (a, b)
        assert not holds(outs["plain"]), (a, b)
        exp = torch.zeros(P)
        O.reduce_tensor(exp, [ups[i] for i in hon], [1.0 / 7] * 7)
        S.assert_bitwise(f"robust {a},{b}", {"w": outs["krum"]}, {"w": exp})


# ---------------------------------------------------------------------------- 7. with the guard
def test_krum_with_the_guard():
    """``clip_threshold`` set: the scales are ``guard.clip_scale(sqrt(G_ii))`` of the round's own
    Gram matrix, the scores are those of the SCALED updates (tests/krum_ref.py on fp64 copies
    pre-scaled on the CPU), the model is the oracle's on updates pre-scaled with its tmp_tensor, and
    the round's launches name flame_update_gram and no flame_update_stats.  ``nonfinite="skip"``
    shrinks n and re-checks 2f + 3; ``"raise"`` raises with the records."""
    from flame_amd import engine
    from flame_amd.optimizer import guard
    O = _oracle()
    n, f = 9, 2
    g = torch.Generator().manual_seed(13)
    ups, honest = _model(g, n, f, torch.float32, True)
    n_el = 4099 + 210
    gram, _ = engine.update_gram([S.to_dev(u, DEV) for u in ups], DEV)
    norms = sorted(math.sqrt(x) for x in gram.diagonal())
    clip = (norms[3] + norms[4]) / 2                         # the larger honest norms and the bad ones are clipped
    base = {"k0": torch.randn(4099, generator=g), "k1": torch.randn(210, generator=g), "nbt": torch.tensor(7)}
    opt = _drop_in("fedavg", krum=f, clip_threshold=clip)
    dev = S.to_dev(base, DEV)
    with _Launches() as ln:
        out = opt.do(dev, _fill([S.to_dev(u, DEV) for u in ups]), total=n)
    assert ln.count("flame_update_gram") == 1 and ln.count("flame_update_stats") == 0, ln.names
    assert ln.count("flame_agg_reduce_scaled") >= 1, ln.names
    scales = [r.scale for r in opt.update_stats]
    assert scales == [guard.clip_scale(math.sqrt(float(gram[i, i])), clip) for i in range(n)]
    assert sum(1 for s in scales if s < 1.0) >= 5 and any(s == 1.0 for s in scales)
    assert [r.norm for r in opt.update_stats] == [math.sqrt(float(gram[i, i])) for i in range(n)]
    ref_scores, ref_sel, _, _ = R.krum(ups, f, scales=scales)
    sel = [i for i, r in enumerate(opt.krum_records) if r.selected]
    assert sel == ref_sel
    _check_scores("clip", opt.krum_records, ref_scores, n - f - 2, n_el, ups, scales)
    exp = S.to_cpu(base)
    pre = [{k: (O.tmp_tensor(v, scales[i]) if v.is_floating_point() else v.clone()) for k, v in ups[i].items()} for i in sel]
    O.OracleFedAvg().do(exp, _fill(pre), total=len(sel))
    S.assert_bitwise("clip", {k: out[k] for k in base}, exp)
    # skip: 8 updates, one all-NaN: n = 7 = 2f + 3 remains and the round runs without it
    ups8, _ = _model(g, 8, 2, torch.float32, True)
    nan_at = 2
    assert nan_at not in R.bad_positions(8, 2)
    ups8[nan_at] = {k: (torch.full_like(v, float("nan")) if v.is_floating_point() else v) for k, v in ups8[nan_at].items()}
    rest = [u for i, u in enumerate(ups8) if i != nan_at]
    opt = _drop_in("fedavg", krum=2, nonfinite="skip")
    dev = S.to_dev(base, DEV)
    out = opt.do(dev, _fill([S.to_dev(u, DEV) for u in ups8]), total=8)
    _, ref_sel, _, _ = R.krum(rest, 2)
    kept = [i for i in range(8) if i != nan_at]
    assert [i for i, r in enumerate(opt.krum_records) if r.selected] == [kept[j] for j in ref_sel]
    assert [r.skipped for r in opt.update_stats] == [i == nan_at for i in range(8)]
    exp = S.to_cpu(base)
    O.OracleFedAvg().do(exp, _fill([S.to_cpu(rest[j]) for j in ref_sel]), total=len(ref_sel))
    S.assert_bitwise("skip", {k: out[k] for k in base}, exp)
    # skip: 7 updates, one all-NaN: 6 < 2f + 3 remain
    cache = _fill([S.to_dev(u, DEV) for u in ups8[:7]])
    dev = S.to_dev(base, DEV)
    with pytest.raises(ValueError, match=r"2f \+ 3"):
        _drop_in("fedavg", krum=2, nonfinite="skip").do(dev, cache, total=7)
    S.assert_bitwise("skip too few", {k: dev[k] for k in base}, S.to_cpu(base))
    # raise
    opt = _drop_in("fedavg", krum=2, nonfinite="raise")
    dev = S.to_dev(base, DEV)
    with pytest.raises(ValueError, match=f"e{nan_at:04d}"):
        opt.do(dev, _fill([S.to_dev(u, DEV) for u in ups8]), total=8)
    assert [r.nonfinite > 0 for r in opt.update_stats] == [i == nan_at for i in range(8)]
    S.assert_bitwise("raise leaves base", {k: dev[k] for k in base}, S.to_cpu(base))
    # keep (the default): the NaN update is ineligible, never selected; all ineligible -> None
    opt = _drop_in("fedavg", krum=2)
    dev = S.to_dev(base, DEV)
    out = opt.do(dev, _fill([S.to_dev(u, DEV) for u in ups8]), total=8)
    assert out is dev and not opt.krum_records[nan_at].selected and math.isinf(opt.krum_records[nan_at].score)
    allnan = [{k: (torch.full_like(v, float("nan")) if v.is_floating_point() else v) for k, v in u.items()} for u in ups8[:7]]
    dev = S.to_dev(base, DEV)
    assert opt.do(dev, _fill([S.to_dev(u, DEV) for u in allnan]), total=7) is None
    S.assert_bitwise("all ineligible", {k: dev[k] for k in base}, S.to_cpu(base))


# ---------------------------------------------------------------------------- 8. residency
def test_host_resident_base_and_pinned_updates_give_the_same_bits():
    g = torch.Generator().manual_seed(21)
    ups, honest = _model(g, 9, 2, torch.float32, True)
    base = {"k0": torch.randn(4099, generator=g), "k1": torch.randn(210, generator=g), "nbt": torch.tensor(7)}
    hbm = S.to_dev(base, DEV)
    o1 = _drop_in("fedavg", krum=2)
    o1.do(hbm, _fill([S.to_dev(u, DEV) for u in ups]), total=9)
    host = {k: v.clone() for k, v in base.items()}
    pinned = [{k: v.clone().pin_memory() for k, v in u.items()} for u in ups]
    before = [{k: v.clone() for k, v in u.items()} for u in pinned]
    o2 = _drop_in("fedavg", krum=2)
    out = o2.do(host, _fill(pinned), total=9)
    assert out is host and all(not v.is_cuda for v in out.values())
    S.assert_bitwise("host base / pinned updates", out, S.to_cpu(hbm))
    exp = S.to_cpu(base)
    _oracle().OracleFedAvg().do(exp, _fill([S.to_cpu(ups[i]) for i in honest]), total=len(honest))
    S.assert_bitwise("host base / oracle", out, exp)
    assert [r.score for r in o1.krum_records] == [r.score for r in o2.krum_records]
    assert [i for i, r in enumerate(o2.krum_records) if r.selected] == honest
    for b, a in zip(before, pinned):
        assert all(torch.equal(b[k], a[k]) for k in b), "an update was written"


# ---------------------------------------------------------------------------- 9. refusals on the device path
def test_refusals_with_nothing_popped():
    from flame_amd import _native
    ups = [{"w": torch.full((4,), float(i), device=DEV)} for i in range(1025)]
    cache = _fill(ups)
    base = {"w": torch.zeros(4, device=DEV)}
    with pytest.raises(NotImplementedError, match="1024"):
        _drop_in("fedavg", krum=1).do(base, cache, total=1025)
    assert len(cache) == 1025 and float(base["w"].abs().sum()) == 0
    cache = _fill(ups[:9])
    with pytest.raises(NotImplementedError, match="Krum"):
        _drop_in("fedavg", krum=1).do(base, cache, total=9, flame_amd_key_groups=[["w"]])
    assert len(cache) == 9
    before = _native.launch_branch_counts()
    assert len(before) == 100
    from flame_amd import engine
    gram, nf = engine.update_gram(ups[:1024], DEV)           # the largest round: 16 tiles, 136 tile pairs
    idx = np.arange(1024, dtype=np.float64)
    assert np.array_equal(gram, 4.0 * np.outer(idx, idx)) and not nf.any()
    opt = _drop_in("fedavg", krum=1)
    out = opt.do(base, _fill(ups[:1024]), total=1024)
    assert out is base and bool(torch.isfinite(base["w"]).all())
    assert sum(1 for r in opt.krum_records if r.selected) == 1023 and not opt.krum_records[1023].selected
    exp = torch.zeros(4)
    _oracle().reduce_tensor(exp, [u["w"].cpu() for u in ups[:1023]], [1.0 / 1023] * 1023)
    S.assert_bitwise("1024 updates", {"w": base["w"]}, {"w": exp})
    assert _native.launch_branch_counts().keys() == before.keys()
