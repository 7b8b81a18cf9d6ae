"""tests/rfa_ref.py against closed forms of the geometric median, and flame_amd/optimizer/rfa.py's
host arithmetic against it (no GPU)."""
import math

import numpy as np
import pytest
import torch

import rfa_ref as R


def test_collinear_points_give_the_median():
    direction = np.array([3.0, -4.0, 12.0]) / 13.0
    pos = [0.5, 1.0, 2.0, 3.0, 10.0]                     # the median of the positions is 2
    xs = [p * direction for p in pos]
    w, trace = R.geomedian(xs, 200)
    z = R.combine(xs, w)
    assert np.linalg.norm(z - 2.0 * direction) < 1e-5
    assert len(trace) == 200 and abs(math.fsum(w) - 1.0) < 1e-15
    assert w[2] > 0.99                                    # the weight gathers on the median point
    # the mean would sit at 3.3: the outlier at 10 does not drag the median
    assert abs(np.dot(z, direction) - 2.0) < 1e-5 < abs(np.mean(pos) - 2.0)


def test_a_symmetric_configuration_gives_the_centroid():
    c = np.array([0.3, -0.2, 0.1, 0.7])
    xs = [c + s * e for e in np.eye(4) for s in (1.0, -1.0)]
    w, _ = R.geomedian(xs, 60)
    assert np.linalg.norm(R.combine(xs, w) - c) < 1e-12
    assert max(w) - min(w) < 1e-12                        # all at distance 1 of the centroid


def test_one_update_is_itself_and_identical_updates_get_equal_weights():
    x = np.array([1.0, -2.0, 0.5])
    for T in (1, 2, 5):
        w, trace = R.geomedian([x], T)
        assert w == [1.0] and np.array_equal(R.combine([x], w), x)
        assert trace[-1][0] == ((0.0,) if T > 1 else (5.25,))
    for n in (2, 3, 7):
        w, _ = R.geomedian([x] * n, 4)
        assert len(set(w)) == 1 and abs(w[0] - 1.0 / n) < 1e-16
    # at the centre itself every distance is below nu: the floor makes the weights equal, not 0 / 0
    assert R.weights([0.0, 0.0, 0.0], 1e-6, None) == [1.0 / 3] * 3


def test_weights_statement():
    w = R.weights([4.0, 16.0, math.inf, math.nan], 1e-6, None)
    assert w[2] == 0.0 and w[3] == 0.0 and w[0] == (1 / 2) / math.fsum([1 / 2, 1 / 4]) and w[1] == (1 / 4) / 0.75
    assert R.weights([1e-20, 1.0], 1e-6, None) == [1e6 / (1e6 + 1.0), 1.0 / (1e6 + 1.0)]      # the floor nu
    prev = [0.25, 0.75]
    assert R.weights([math.inf, math.nan], 1e-6, prev) == prev                              # every beta 0
    from flame_amd.optimizer import rfa
    for d2 in ([4.0, 16.0, math.inf, math.nan], [1e-20, 1.0], [0.0, 0.0], [3.0], [math.inf, math.nan]):
        assert rfa.weights(d2, 1e-6, [1.0 / len(d2)] * len(d2)) == R.weights(d2, 1e-6, [1.0 / len(d2)] * len(d2))


def test_dist2_statement():
    ups = [{"a": torch.tensor([1.0, 2.0, float("nan")]), "i": torch.tensor([7]), "b": torch.tensor([0.5], dtype=torch.float64)},
           {"a": torch.tensor([float("inf"), 2.0, 3.0]), "i": torch.tensor([7]), "b": torch.tensor([1e308], dtype=torch.float64)}]
    z = {"a": torch.tensor([0.5, 2.0, 1.0]), "b": torch.tensor([-1e308], dtype=torch.float64)}
    d2, bad = R.dist2(ups, z)
    assert bad == [1, 1] and d2[0] == math.inf and d2[1] == math.inf        # 0.5 + 1e308 squared overflows
    z["b"] = torch.tensor([0.25], dtype=torch.float64)
    d2, bad = R.dist2(ups[:1], z)
    assert d2 == [0.25 + 0.0625] and bad == [1]
    z["a"] = torch.tensor([float("inf"), 2.0, float("nan")])
    assert R.dist2(ups, z)[0][0] == math.inf                                # finite there: +inf
    assert R.dist2(ups[1:], {"a": z["a"], "b": torch.tensor([1e308], dtype=torch.float64)})[0] == [math.nan]


@pytest.mark.parametrize("n,bad", [(9, 3), (33, 12)])
def test_the_attack_round(n, bad):
    """The conditions the GPU test asserts of FedAvg(rfa=5), on the fp64 reference alone."""
    for seed in (0, 1, 2):
        g = torch.Generator().manual_seed(100 * n + seed)
        ups, pos, honest = R.attack_round(g, n, bad)
        xs = [u.double().numpy() for u in ups]
        w, _ = R.geomedian(xs, 5)
        plain = np.mean(xs, axis=0)
        ratio = np.linalg.norm(R.combine(xs, w) - honest) / np.linalg.norm(plain - honest)
        colluders = math.fsum(w[i] for i in pos)
        print(f"n={n} bad={bad} seed={seed}: ratio {ratio:.4f}, colluders' weight {colluders:.4f}")
        assert ratio < 0.25 and colluders < 0.1
