"""GPU: the low-rank downlink (flame_lowrank_factor, engine.lowrank_factor, MessageEncoder(lowrank=)) against a plain fp64
numpy restatement of DESIGN.md §2, "the low-rank downlink": P = D Q, U = orth(P), V = U^T D on D = W - base.  Every bound is
derived from u = 2^-24, the fp32 unit roundoff, and the length summed over; none from what the kernels give."""
from collections import OrderedDict

import cloudpickle
import numpy as np
import pytest
import torch

from flame_amd import egress, engine, lowrank
from large_case import Launches
from lowrank_ref import gamma
from oracle import consult

pytestmark = [pytest.mark.gpu]
oracle = pytest.mark.oracle
DEV, U32 = "cuda:0", 2.0 ** -24
# one row, one column; below, at and above the instruction's 32 and the tile's 128; 257 is five stages of K; a 4-D key
SHAPES = [(1, 33), (33, 1), (31, 32), (32, 31), (33, 129), (127, 128), (128, 127), (128, 128), (129, 257), (257, 129), (257, 257),
          (257, 32), (3, 5, 2, 7)]
F64 = lambda t: t.detach().cpu().numpy().astype(np.float64)      # noqa: E731


def _case(kind, rank, g):
    """{key: (W, base)} fp32 CPU tensors and q (None: the noise start).  exact: D = A B of small integers, A = [I; ..] and
    B = [I, ..], so of rank min(rank, m, n) exactly; ulp: q's first two columns differ by one ulp; zero: W == base."""
    keys, q = OrderedDict(), {}
    for i, shape in enumerate(SHAPES):
        m, n = lowrank.matrix_shape(shape)
        r = min(rank, m, n)
        if kind == "exact":
            base = torch.randint(-8, 9, (m, n), generator=g).float()
            a, c = torch.randint(-4, 5, (m, r), generator=g).float(), torch.randint(-4, 5, (r, n), generator=g).float()
            a[:r], c[:, :r] = torch.eye(r), torch.eye(r)       # both factors of full rank whatever was drawn
            d = a @ c
        else:
            base = torch.randn(m, n, generator=g) * 4
            d = torch.zeros(m, n) if kind == "zero" else torch.randn(m, n, generator=g) * torch.exp2(torch.randint(-6, 3, (m, 1), generator=g).float())
        keys[f"k{i}"] = ((base + d).view(shape), base)
        if kind == "ulp":
            q[f"k{i}"] = torch.randn(n, r, generator=g)
            if r > 1:
                q[f"k{i}"][:, 1] = torch.nextafter(q[f"k{i}"][:, 0], torch.tensor(float("inf")))
    return keys, (q if kind == "ulp" else None)


def _factor(keys, q, rank):
    """One engine.lowrank_factor call; key k3 is host-resident.  Returns (sent, q_next, {key: advanced base})."""
    weights = OrderedDict((k, w if k == "k3" else w.to(DEV)) for k, (w, _) in keys.items())
    weights["steps"] = torch.tensor([3])
    base = {k: b.to(DEV).reshape(-1) for k, (_, b) in keys.items()}
    with Launches() as ln:
        sent, q_next = engine.lowrank_factor(weights, rank, base=base, q=q and {k: t.to(DEV) for k, t in q.items()}, seed=11)
    assert [n for n in ln.names if n != "flame_noise_fill"] == ["flame_lowrank_factor", "flame_agg_reduce_lowrank"], ln.names
    assert sent["steps"] is weights["steps"] and set(sent.right) == set(keys) == set(q_next)
    return sent, q_next, base


@oracle
@pytest.mark.parametrize("items", [512, 40, 1], ids=lambda i: f"items{i}")       # every stage its own split; ragged splits; one split
@pytest.mark.parametrize("rank", [1, 4, 16, 32])
@pytest.mark.parametrize("kind", ["random", "exact", "ulp", "zero"])
def test_factors_against_the_fp64_restatement(kind, rank, items, monkeypatch):
    monkeypatch.setattr(engine, "LOWRANK_FACTOR_ITEMS", items)
    keys, q = _case(kind, rank, torch.Generator().manual_seed(100 * rank + items))
    (sent, q_next, adv), (sent2, q_next2, _) = _factor(keys, q, rank), _factor(keys, q, rank)
    consult.note()
    # the start the call took: q, or the noise of (seed, the key's position in weights)
    start = q or engine.noise_fill(OrderedDict((k, v.t()) for k, v in sent.right.items()), 11, 0, 1.0, device=DEV)
    worst = {"orth": 0.0, "proj": 0.0, "rank": 0.0, "base": 0.0}
    for k, (w, b) in keys.items():
        m, n = lowrank.matrix_shape(w.shape)
        r = min(rank, m, n)
        U, V, D, B = F64(sent[k]), F64(sent.right[k]), F64(w).reshape(m, n) - F64(b), F64(b)
        assert U.shape == (m, r) and V.shape == (r, n) and sent.shapes[k] == tuple(w.shape), k
        assert np.isfinite(U).all() and np.isfinite(V).all(), f"{k}: a factor is not finite"
        for a, c in ((sent[k], sent2[k]), (sent.right[k], sent2.right[k]), (q_next[k], q_next2[k])):       # determinism: equal bits
            assert torch.equal(a.contiguous().view(torch.int32), c.contiguous().view(torch.int32)), k
        assert torch.equal(q_next[k], sent.right[k].t()), k
        if kind == "zero":
            assert not U.any() and not V.any() and torch.equal(adv[k].cpu(), b.reshape(-1)), f"{k}: zero change"
            continue
        # Orthogonality.  A stored column is an exact projection (fp64: its error is 2^-29 of u) rounded to fp32 element by
        # element twice, as the residual and as the normalised column: |u_k . u_c| <= 2 u by Cauchy-Schwarz, and
        # |u_c . u_c - 1| <= 2 u.  The re-orthogonalisation subtracts along c <= r earlier columns that are themselves orthogonal
        # only to 2 u, with coefficients no larger than the column: 2 u more per earlier column.  (2 + 2 r) u <= 4 r u.
        G = U.T @ U
        diag = np.rint(np.diag(G))
        assert set(diag) <= {0.0, 1.0} and not U[:, diag == 0].any() and diag.all(), f"{k}: diag {np.diag(G)}"
        worst["orth"] = max(worst["orth"], np.abs(G - np.diag(diag)).max() / (4 * r * U32))
        # Projection: a sum of m products in any order over D = f32(w - base), one more rounding: gamma_{m+1}; one spare.
        pb = gamma(m + 2) * (np.abs(U).T @ np.abs(D))
        worst["proj"] = max(worst["proj"], (np.abs(V - U.T @ D) / np.maximum(pb, 1e-300)).max())
        # The base advanced by the uplink's launch: its bound, gamma_{r+1} (|in| + |U| |V|), r padded to even (two zeros more).
        ab = gamma(r + 3) * (np.abs(B) + np.abs(U) @ np.abs(V))
        worst["base"] = max(worst["base"], (np.abs(F64(adv[k]).reshape(m, n) - (B + U @ V)) / np.maximum(ab, 1e-300)).max())
        if kind == "exact":
            # Exact rank: range(D) = range(P) for P = D Q of full column rank, so D = P C with C = pinv(P) D, and
            # (I - U U^T) D = (I - U U^T)(E + F) C, E the product's error on P, |E| <= gamma_{n+1} |D| |Q| (any order, plus the
            # subtract), F the backward error of Gram-Schmidt, ||F|| <= 4 r u ||P|| by the count above.  ||I - U U^T|| <= 1 + r 4 r u
            # < 2.  The second term is U times V's error, ||U|| < 2.
            P = D @ F64(start[k])
            s = np.linalg.svd(P, compute_uv=False)
            assert s[-1] > 1e-6 * s[0], f"{k}: the case is not of full rank"
            tol = 2 * np.linalg.norm(np.linalg.pinv(P) @ D, 2) * (gamma(n + 1) * np.linalg.norm(np.abs(D) @ np.abs(F64(start[k]))) + 4 * r * U32 * np.linalg.norm(P)) \
                + 2 * np.linalg.norm(pb)
            worst["rank"] = max(worst["rank"], np.linalg.norm(D - U @ V) / tol)
    print(f"{kind} r={rank} items={items}: worst fractions of the bounds {worst}")
    assert all(v <= 1.0 for v in worst.values()), worst


def test_noise_start_is_the_keys_stream():
    """Without q the start is noise_fill of (seed, the key's position in weights): the first message is reproducible."""
    w = OrderedDict(a=torch.tensor([1]), b=torch.randn(40, 50, device=DEV))
    sent, _ = engine.lowrank_factor(w, 4, base={"b": torch.zeros(2000, device=DEV)}, seed=9)
    q = engine.noise_fill(w, 9, 0, 1.0, device=DEV)["b"].reshape(-1)[:200].view(50, 4)      # stream 1: b's position
    again, _ = engine.lowrank_factor(w, 4, base={"b": torch.zeros(2000, device=DEV)}, q={"b": q})
    assert torch.equal(sent["b"], again["b"]) and torch.equal(sent.right["b"], again.right["b"])


@oracle
def test_encoder_rounds():
    g = torch.Generator().manual_seed(3)
    W, r = torch.randn(129, 65, generator=g), 4
    model = OrderedDict(w=W.to(DEV), steps=torch.tensor([5, 6]))
    for kw in ({"mx": "e4m3"}, {"sparse": 0.1}):
        with pytest.raises(ValueError, match="choose one"):
            egress.MessageEncoder(lowrank=r, **kw)
    enc = egress.MessageEncoder(lowrank=r, lowrank_seed=2)
    trainer, bound, norms = {}, 0.0, []
    consult.note()
    for rnd in range(5):
        if rnd == 1:
            model["w"] = (W * 1.5 + 1).to(DEV)              # the target moves once, then stays
        if rnd == 4:
            enc.reset()
        msg = cloudpickle.loads(enc.encode_bytes({"weights": model, "round": rnd}))["weights"]
        assert isinstance(msg, lowrank.LowRankWeights) == (rnd not in (0, 4)) and torch.equal(msg["steps"], model["steps"]), rnd
        held, prev = (F64(trainer["w"]), base) if rnd else (None, None)
        lowrank.apply_(trainer, msg)
        base = F64(enc._base["w"])
        if rnd in (0, 4):
            assert torch.equal(trainer["w"], model["w"].cpu()) and np.array_equal(base, F64(trainer["w"]))
            bound = 0.0
        else:
            # both sides add U V to what they hold, each within gamma_{r+3} (|held| + |U| |V|) of the exact sum (the encoder's k
            # is padded to even, the trainer's product is rounded once more): the bounds add up from message to message
            U, V = F64(msg["w"]), F64(msg.right["w"])
            step = gamma(r + 3) * (np.abs(prev) + np.abs(U) @ np.abs(V))
            bound = bound + step + gamma(r + 3) * (np.abs(held) + np.abs(U) @ np.abs(V))
            assert (np.abs(F64(trainer["w"]) - base) <= bound).all(), rnd
        norms.append(np.linalg.norm(F64(model["w"]) - base))
        if rnd in (2, 3):
            # error feedback with the target fixed: W - base' = D - U V up to `step`, and D - U V = (I - U U^T) D + U (U^T D - V):
            # ||I - U U^T|| <= 1 + 4 r^2 u by the orthogonality bound, V's error is gamma_{m+2} |U|^T |D| and ||U|| < 2
            D = F64(model["w"]) - prev
            slack = 4 * r * r * U32 * norms[-2] + 2 * np.linalg.norm(gamma(129 + 2) * np.abs(U).T @ np.abs(D)) + np.linalg.norm(step)
            assert norms[-1] <= norms[-2] + slack, norms
    assert norms[0] == 0.0 and norms[4] == 0.0 and norms[1] > 0.0
