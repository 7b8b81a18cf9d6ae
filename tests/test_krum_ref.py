"""Krum on the CPU: the package's Gram route (``flame_amd/optimizer/krum.py`` on ``X X^T``) against the
direct route of tests/krum_ref.py (``sum (x_i - x_j)^2``), both on data verified here.

* On exact-sum inputs (integers in [-8, 8]: every product and partial sum is exact in fp64) the two
  routes give bitwise equal distances, scores and selections.
* On honest-plus-bad rounds the selected set is exactly the honest set, the relative gap between the
  m-th and the (m + 1)-th score is >= 0.99, and the two routes' scores differ by <= 5.2e-14 relative.
"""
import math

import numpy as np
import pytest
import torch

import krum_ref as R

ROUNDS = [(5, 1), (9, 2), (17, 4), (33, 8), (65, 16), (130, 31)]
SIZES = [1023, 1025, 4099]


def _gram(ups):
    """The correctly rounded Gram matrix (math.fsum of the fp64 products): what the Gram route loses
    against the direct one is then the route's own cancellation, not a summation order."""
    flat = [R.flatten(u) for u in ups]
    n = len(flat)
    gram = np.empty((n, n))
    for i in range(n):
        for j in range(i, n):
            gram[i, j] = gram[j, i] = math.fsum(flat[i][0] * flat[j][0])
    return gram, np.asarray([bad for _, bad in flat], np.int64)


@pytest.mark.parametrize("nf", ROUNDS, ids=[f"n{n}f{f}" for n, f in ROUNDS])
def test_exact_sum_inputs_both_routes_bitwise(nf):
    from flame_amd.optimizer import krum
    n, f = nf
    g = torch.Generator().manual_seed(100 + n)
    ups = R.integer_updates(g, n, (257, 0, 1, 300))
    gram, nonfinite = _gram(ups)
    assert np.array_equal(gram, R.exact_gram(ups))
    d_ref, nf_ref = R.distances(ups)
    d, eligible = krum.distances(gram, nonfinite, None)
    assert eligible.all() and np.array_equal(nonfinite, nf_ref)
    assert np.array_equal(d.view(np.uint64), d_ref.view(np.uint64))
    for m in (None, 1, n - f):
        sc_ref, sel_ref = R.select(d_ref, f, m)
        sc, sel = krum.select(gram, nonfinite, None, f, n - f if m is None else m)
        assert np.array_equal(np.asarray(sc).view(np.uint64), np.asarray(sc_ref).view(np.uint64))
        assert sel == sel_ref and len(sel) == (n - f if m is None else m)
    # clip scales that are powers of two keep everything exact
    scales = [0.5 if i % 3 == 0 else 1.0 for i in range(n)]
    d_ref, _ = R.distances(ups, scales)
    d, _ = krum.distances(gram, nonfinite, scales)
    assert np.array_equal(d.view(np.uint64), d_ref.view(np.uint64))


@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("nf", ROUNDS, ids=[f"n{n}f{f}" for n, f in ROUNDS])
def test_honest_plus_bad_selects_exactly_the_honest_set(nf, P):
    from flame_amd.optimizer import krum
    n, f = nf
    g = torch.Generator().manual_seed(7 * n + P)
    ups, honest = R.honest_bad(g, n, f, (P,))
    gram, nonfinite = _gram(ups)
    sc, sel = krum.select(gram, nonfinite, None, f, n - f)
    sc_ref, sel_ref, _, _ = R.krum(ups, f)
    assert sel == honest and sel_ref == honest
    ranked = sorted(sc)
    m = n - f
    gap = (ranked[m] - ranked[m - 1]) / ranked[m]
    rel = max(abs(a - b) / b for a, b in zip(sc, sc_ref))
    print(f"n={n} f={f} P={P}: gap {gap:.4f}, routes differ by {rel:.3e} relative")
    assert gap >= 0.99
    assert rel <= 5.2e-14
    # Krum proper: the single lowest score, an honest update
    _, one = krum.select(gram, nonfinite, None, f, 1)
    assert one == [int(np.argmin(sc))] and one[0] in honest


def test_a_one_element_key_is_not_part_of_the_property():
    """At P = 1 the honest set is not separated (a bad draw can land inside the honest spread):
    only the routes' agreement is asserted there."""
    from flame_amd.optimizer import krum
    g = torch.Generator().manual_seed(3)
    ups, _ = R.honest_bad(g, 9, 2, (1,))
    gram, nonfinite = _gram(ups)
    sc, sel = krum.select(gram, nonfinite, None, 2, 7)
    sc_ref, sel_ref, _, _ = R.krum(ups, 2)
    assert len(sel) == 7 and all(math.isfinite(x) for x in sc)
    assert all(abs(a - b) <= 1e-9 * max(abs(b), 1e-300) + 1e-15 for a, b in zip(sc, sc_ref))
